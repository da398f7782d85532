"""MXFP8 kernels against their per-tensor counterparts on one GPU.

GEMM: ``gemm_mxfp8`` vs ``gemm_fp8`` (bf16 output, no epilogue extras) on the ViT-B/16 linear shapes at the
benchmark batch (tokens = 128 x 197) and at 8192^3, as TF/s from 2 M N K over device-event time.
Quantiser: ``mx_quantize`` (both orientations) vs ``fp8_quantize_both_delayed`` on the [tokens, 768] and
[tokens, 3072] activations, as GB/s of the bytes each must move (one bf16 read, two e4m3 writes, plus MX scales).
MLP epilogue: ``gemm_mxfp8_quant_out`` on the two [tokens, 3072] x 768 MLP GEMMs (act 2 and act 3) vs the passes it
replaces and vs the GEMM alone.
LayerNorm: ``layernorm_fwd_mx`` vs ``layernorm_fwd`` + ``mx_quantize``, and ``layernorm_bwd_mx`` vs ``layernorm_bwd`` +
``mx_quantize`` + ``colsum_f32`` (and vs ``layernorm_bwd`` alone), at [128 x 197, 768] and [32 x 577, 768].
The variants of a row are timed alternately, ``--rounds`` windows each; the median and the spread are printed.
One JSON line per row.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ringdp._native import C  # noqa: E402


def _time(fn, iters: int) -> float:
    """Milliseconds per call over ``iters`` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _pair(f_mx, f_pt, iters: int, rounds: int):
    for f in (f_mx, f_pt):  # warm-up: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t_mx, t_pt = [], []
    for _ in range(rounds):
        t_mx.append(_time(f_mx, iters))
        t_pt.append(_time(f_pt, iters))
    return t_mx, t_pt


def _stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def bench_gemm(M: int, N: int, K: int, splits: int, iters: int, rounds: int) -> dict:
    a = torch.randn(M, K, device="cuda").bfloat16()
    b = torch.randn(N, K, device="cuda").bfloat16()
    aq, sa, _, _ = C.mx_quantize(a, True, False)
    bq, sb, _, _ = C.mx_quantize(b, True, False)
    pa, _, psa = C.fp8_quantize_both(a)
    pb, _, psb = C.fp8_quantize_both(b)
    Kp = aq.shape[1]
    if splits > 1:  # a weight gradient: split-K into fp32
        out = torch.empty(M, N, device="cuda")
        t_mx, t_pt = _pair(lambda: C.gemm_mxfp8_splitk_f32(aq, sa, bq, sb, M, N, Kp, splits, out),
                           lambda: C.gemm_fp8_splitk_f32(pa, pb, psa, psb, M, N, K, splits, out), iters, rounds)
    else:
        t_mx, t_pt = _pair(lambda: C.gemm_mxfp8(aq, sa, bq, sb, M, N, Kp, True),
                           lambda: C.gemm_fp8(pa, pb, psa, psb, M, N, K, True), iters, rounds)
    flop = 2.0 * M * N * K
    (m, lo, hi), (p, plo, phi) = _stats(t_mx), _stats(t_pt)
    return {"kind": "gemm", "M": M, "N": N, "K": K, "splits": splits, "mx_ms": round(m, 4), "mx_ms_range": [round(lo, 4), round(hi, 4)],
            "tensor_ms": round(p, 4), "tensor_ms_range": [round(plo, 4), round(phi, 4)],
            "mx_tflops": round(flop / m / 1e9, 1), "tensor_tflops": round(flop / p / 1e9, 1)}


def bench_quant(R: int, Cc: int, iters: int, rounds: int) -> dict:
    x = torch.randn(R, Cc, device="cuda").bfloat16()
    hist = torch.zeros(1 + C.fp8_delayed_slots(R, Cc), device="cuda")
    C.fp8_quantize_both_delayed(x, hist, True)  # the site's first call measures the amax
    t_mx, t_pt = _pair(lambda: C.mx_quantize(x, True, True),
                       lambda: C.fp8_quantize_both_delayed(x, hist, False, roll=False), iters, rounds)
    byt = R * Cc * (2 + 2)
    (m, lo, hi), (p, plo, phi) = _stats(t_mx), _stats(t_pt)
    return {"kind": "quant", "R": R, "C": Cc, "mx_ms": round(m, 4), "mx_ms_range": [round(lo, 4), round(hi, 4)],
            "tensor_ms": round(p, 4), "tensor_ms_range": [round(plo, 4), round(phi, 4)],
            "mx_gbs": round((byt + 2 * R * Cc / 32) / m / 1e6, 1), "tensor_gbs": round(byt / p / 1e6, 1)}


def bench_mlp(M: int, N: int, K: int, act: int, iters: int, rounds: int) -> dict:
    """The MXFP8-writing epilogue on an MLP GEMM (act 2: fc1 forward with bias; act 3: fc2's data gradient with the
    column sums) against the passes it replaces - the GEMM to bf16, ``mx_quantize`` of its output and, for act 3,
    ``gelu_bwd`` and ``colsum_f32`` - and against that GEMM alone."""
    a = torch.randn(M, K, device="cuda").bfloat16()
    b = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    aq, sa, _, _ = C.mx_quantize(a, True, False)
    bq, sb, _, _ = C.mx_quantize(b, True, False)
    Kp = aq.shape[1]
    pre = torch.randn(M, N, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda") if act == 2 else None
    cs = torch.empty(N, device="cuda") if act == 3 else None

    def fused():
        C.gemm_mxfp8_quant_out(aq, sa, bq, sb, M, N, Kp, bias, act, pre, cs)

    def gemm_only():
        return C.gemm_mxfp8(aq, sa, bq, sb, M, N, Kp, True, bias, 2 if act == 2 else 0, None, pre if act == 2 else None)

    def passes():
        y = gemm_only()
        if act == 3:
            y = C.gelu_bwd(y, pre)
            C.colsum_f32(y, cs)
        C.mx_quantize(y, True, True)

    fns = (fused, passes, gemm_only)
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[], [], []]
    for _ in range(rounds):  # alternating windows
        for t, f in zip(ts, fns):
            t.append(_time(f, iters))
    out = {"kind": "mlp_epilogue", "M": M, "N": N, "K": K, "act": act}
    for name, t in zip(("fused", "passes", "gemm_only"), ts):
        m, lo, hi = _stats(t)
        out[name + "_ms"] = round(m, 4)
        out[name + "_ms_range"] = [round(lo, 4), round(hi, 4)]
    return out


def bench_ln(R: int, D: int, iters: int, rounds: int) -> dict:
    """``layernorm_fwd_mx`` (both orientations) against the two calls it replaces, ``layernorm_fwd`` and
    ``mx_quantize`` of its rows.  GB/s from the bytes each must move: the fused call reads x (bf16) and writes two
    e4m3 copies and their scales; the two calls also write the bf16 rows and read them back."""
    x = torch.randn(R, D, device="cuda").bfloat16()
    w, b = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")

    def passes():
        C.mx_quantize(C.layernorm_fwd(x, w, b, 1e-6)[0], True, True)

    t_f, t_p = _pair(lambda: C.layernorm_fwd_mx(x, w, b, 1e-6, True), passes, iters, rounds)
    byt = R * D * (2 + 2) + 2 * R * D / 32
    (m, lo, hi), (p, plo, phi) = _stats(t_f), _stats(t_p)
    return {"kind": "layernorm", "R": R, "D": D, "fused_ms": round(m, 4), "fused_ms_range": [round(lo, 4), round(hi, 4)],
            "passes_ms": round(p, 4), "passes_ms_range": [round(plo, 4), round(phi, 4)],
            "fused_gbs": round(byt / m / 1e6, 1), "passes_gbs": round((byt + R * D * 4) / p / 1e6, 1)}


def bench_ln_bwd(R: int, D: int, iters: int, rounds: int) -> dict:
    """``layernorm_bwd_mx`` (both orientations, band column sums) against the three calls it replaces,
    ``layernorm_bwd``, ``mx_quantize`` and ``colsum_f32`` of its dx, and against ``layernorm_bwd`` alone (what the
    MXFP8 outputs cost on top), in alternating windows."""
    x, dy, dres = (torch.randn(R, D, device="cuda").bfloat16() for _ in range(3))
    w = torch.rand(D, device="cuda") + 0.5
    stats = C.layernorm_fwd(x, w, torch.zeros_like(w), 1e-6)[1]
    dw, db, cs = (torch.empty(D, device="cuda") for _ in range(3))

    def passes():
        dx = C.layernorm_bwd(dy, x, stats, w, dres, dw, db)
        C.mx_quantize(dx, True, True)
        C.colsum_f32(dx, cs)

    fns = {"fused": lambda: C.layernorm_bwd_mx(dy, x, stats, w, dres, dw, db, True), "passes": passes,
           "bwd_only": lambda: C.layernorm_bwd(dy, x, stats, w, dres, dw, db)}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):  # alternating windows
        for k, f in fns.items():
            ts[k].append(_time(f, iters))
    out = {"kind": "layernorm_bwd", "R": R, "D": D}
    for k, v in ts.items():
        m, lo, hi = _stats(v)
        out[k + "_ms"] = round(m, 4)
        out[k + "_ms_range"] = [round(lo, 4), round(hi, 4)]
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128, help="images per step (197 tokens each)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-mlp", action="store_true", help="only the MLP-epilogue rows")
    ap.add_argument("--only-ln", action="store_true", help="only the LayerNorm rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp8_bench: needs a GPU")
    T = args.batch * 197
    # forward / data-gradient shapes of qkv, proj, fc1, fc2; two weight gradients (split-K over the tokens, the
    # count LinearF asks for); 8192^3
    Tk = T // 128 * 128
    shapes = [(T, 2304, 768, 1), (T, 768, 768, 1), (T, 3072, 768, 1), (T, 768, 3072, 1), (T, 768, 2304, 1),
              (3072, 768, Tk, 4), (768, 3072, Tk, 4), (8192, 8192, 8192, 1)]
    only = args.only_mlp or args.only_ln
    for M, N, K, splits in ([] if only else shapes):
        print(json.dumps(bench_gemm(M, N, K, splits, args.iters, args.rounds)), flush=True)
    for R, Cc in (() if only else ((T, 768), (T, 3072))):
        print(json.dumps(bench_quant(R, Cc, args.iters, args.rounds)), flush=True)
    for act in (() if args.only_ln else (2, 3)):  # fc1 forward, fc2 data gradient: [tokens, 3072] out of K = 768
        print(json.dumps(bench_mlp(T, 3072, 768, act, args.iters, args.rounds)), flush=True)
    for R in (() if args.only_mlp else (T, args.batch // 4 * 577)):  # 224 x 224 at the batch; 384 x 384 at a quarter
        print(json.dumps(bench_ln(R, 768, args.iters, args.rounds)), flush=True)
        print(json.dumps(bench_ln_bwd(R, 768, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
