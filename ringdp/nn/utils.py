"""ringdp.nn.utils - gradient clipping on ringdp kernels.

``clip_grad_norm_`` has ``torch.nn.utils.clip_grad_norm_``'s semantics.  On GPU it is three launches on the current
stream (``grad_sumsq`` -> ``adam_prepare`` -> ``grad_scale_multi``, csrc/kernels/optim.hip) with a fixed reduction
order, so the norm is bitwise reproducible, and it returns the total norm as a device tensor without a host sync.
Optimizers that clip inside their update (``ringdp.optim.AdamW(max_grad_norm=...)``) do not need it.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from .._native import C

_TABLES: "OrderedDict[tuple, tuple]" = OrderedDict()  # gradient addresses -> (table, partials)
_MAX_TABLES = 8


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads or not any(g.is_cuda for g in grads):
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type,
                                              error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"ringdp.nn.utils.clip_grad_norm_: norm_type={norm_type} is not supported on "
                                  "GPU (only the 2-norm)")
    if error_if_nonfinite:
        raise NotImplementedError("ringdp.nn.utils.clip_grad_norm_: error_if_nonfinite=True needs a host sync and "
                                  "is not supported on GPU")
    max_norm = float(max_norm)
    # Pointer table cached per gradient addresses: the synchronous upload happens once per set of gradients.
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    ent = _TABLES.get(key)
    if ent is None:
        table = C.adam_table_build([], grads, [], [], [len(grads)])
        ent = (table, torch.zeros(table.nchunks, dtype=torch.float32, device=grads[0].device))
        _TABLES[key] = ent
        if len(_TABLES) > _MAX_TABLES:
            _TABLES.popitem(last=False)
    else:
        _TABLES.move_to_end(key)
    table, partials = ent
    rec = torch.empty(4, dtype=torch.float32, device=grads[0].device)  # {total_norm, clip_coef, -, -}
    C.grad_sumsq_run(table, partials)
    C.adam_prepare_run(rec, partials, table.nchunks, max_norm, [], [], [])
    C.grad_scale_run(table, rec)
    return rec[0]
