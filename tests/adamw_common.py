"""Shared pieces of the AdamW / Adam tests: shapes, the fp64 torch oracle and the emulated DDP flat layout.

Oracle: ``torch.optim.AdamW`` / ``Adam`` (with ``torch.nn.utils.clip_grad_norm_`` where clipping is on) in fp64 on
CPU copies of the same parameters and gradients.  Gate: the project's optimizer tolerance (test_sgd_matches_torch),
rtol 1e-5 / atol 1e-6 on parameters, exp_avg, exp_avg_sq, and rtol 1e-5 on the norm.  fp32 ``torch.optim.AdamW``
itself stays inside that gate against fp64 over these hyper-parameters (worst abs error 1.6e-6 on |p| ~ 4), so the
gate separates rounding from a wrong formula."""
import torch

RTOL, ATOL = 1e-5, 1e-6

# aligned multiple of 4; scalar tails; one element; one 65536-chunk boundary; a boundary plus a tail
SHAPES = [(10, 2048), (10,), (33,), (1,), (128, 64, 3, 3), (65536 + 7,)]
# (lr, weight_decay)
HYPERS = [(1e-2, 0.0), (1e-3, 1e-2), (3e-2, 5e-2)]
GRAD_SCALES = [0.1, 1.0, 10.0]


def values(shapes, seed=3):
    """Initial parameter values, generated on the CPU so that every device sees the same numbers."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def grads_for(shapes, step, scale, seed=3):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [torch.randn(s, generator=g) * scale for s in shapes]


def leaves(vals, dev, misaligned_last=False):
    """fp32 leaf parameters on ``dev``.  ``misaligned_last``: the last one is a contiguous leaf whose storage
    starts 4 bytes into an allocation (4-byte but not 16-byte aligned), as ``base[1:34]``."""
    ps = [v.to(dev).clone().requires_grad_() for v in vals]
    if misaligned_last:
        v = vals[-1].reshape(-1)
        base = torch.zeros(v.numel() + 8, device=dev)
        base[1:1 + v.numel()].copy_(v)
        p = base[1:1 + v.numel()].detach().requires_grad_()
        assert p.is_leaf and p.is_contiguous() and p.data_ptr() % 16 == 4
        ps[-1] = p
    return ps


class Flat:
    """Emulates DDP flattening exactly as test_sgd_matches_torch does: params and grads become views of flat
    buffers at offsets rounded to 16 elements, with ``_ringdp_flat`` set by hand."""

    def __init__(self, ps):
        dev = ps[0].device
        self.ps, self.offs, tot = ps, [], 0
        for p in ps:
            self.offs.append(tot)
            tot += (p.numel() + 15) // 16 * 16
        self.fp = torch.zeros(tot, device=dev)
        self.fg = torch.zeros(tot, device=dev)
        for p, o in zip(ps, self.offs):
            v = self.fp[o:o + p.numel()].view_as(p)
            v.copy_(p.data)
            p.data = v
            p._ringdp_flat = (self.fp, self.fg, o, len(ps))

    def set_grads(self, grads):
        for p, o, g in zip(self.ps, self.offs, grads):
            view = self.fg[o:o + p.numel()].view_as(p)
            view.copy_(g)
            p.grad = view


def set_grads(ps, grads, misaligned_last=False):
    """Fresh gradient tensors; for a misaligned last parameter the gradient is misaligned too."""
    for p, g in zip(ps, grads):
        p.grad = g.to(p.device).clone().view_as(p)
    if misaligned_last:
        p = ps[-1]
        base = torch.zeros(p.numel() + 8, device=p.device)
        view = base[1:1 + p.numel()]
        view.copy_(grads[-1].reshape(-1))
        p.grad = view
        assert p.grad.data_ptr() % 16 == 4


class Oracle:
    """fp64 torch optimizer on CPU copies; ``groups``: list of (indices, extra group options)."""

    def __init__(self, vals, decoupled, max_norm=None, groups=None, **kw):
        self.ps = [v.double().clone().requires_grad_() for v in vals]
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        if groups is None:
            arg = self.ps
        else:
            arg = [dict(params=[self.ps[i] for i in idx], **opts) for idx, opts in groups]
        self.opt = cls(arg, **kw)
        self.max_norm = max_norm
        self.norm = None

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = g.double().clone().view_as(p)
        if self.max_norm is not None:
            self.norm = torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm)
        self.opt.step()

    def check(self, my_ps, my_opt, what=""):
        for i, (a, r) in enumerate(zip(my_ps, self.ps)):
            st, rst = my_opt.state[a], self.opt.state[r]
            for name, x, y in (("param", a.detach(), r.detach()), ("exp_avg", st["exp_avg"], rst["exp_avg"]),
                               ("exp_avg_sq", st["exp_avg_sq"], rst["exp_avg_sq"])):
                torch.testing.assert_close(x.detach().cpu().double().reshape(-1), y.reshape(-1), rtol=RTOL, atol=ATOL,
                                           msg=lambda m, i=i, name=name: f"{what} tensor {i} {name}: {m}")

    def check_norm(self, norm):
        torch.testing.assert_close(norm.detach().cpu().double().reshape(()), self.norm.reshape(()), rtol=RTOL, atol=0.0)
