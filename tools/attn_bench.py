"""Time the fused attention kernels (head dim 64); the default is the ViT-B/16 B=128 shape (T=197, H=12).
python tools/attn_bench.py [--B 32 --T 577 --H 12] [--unfused-too]

T <= 256 times the stored-P kernels as before; longer sequences time the key-blocked kernels (log-sum-exp form).
--unfused-too also times AttentionF forward and forward + backward on the path in use and on the GEMM path
(ringdp.ops.transformer._ATTN_UNFUSED toggled in-process), in interleaved rounds on the same random data, and
reports the median and the minimum of each plus the peak memory of one forward + backward."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
import ringdp  # noqa: E402

C = ringdp._C


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1000.0


def unfused_too(qkv, dout, B, T, H, fl, rounds=7, iters=5):
    import ringdp.ops.transformer as tr

    x = qkv.clone().requires_grad_()

    def fwd():
        with torch.no_grad():
            tr.AttentionF.apply(x, B, T, H)

    def fwd_bwd():
        x.grad = None
        tr.AttentionF.apply(x, B, T, H).backward(dout)

    saved = tr._ATTN_UNFUSED
    times = {(u, n): [] for u in (False, True) for n in ("fwd", "fwd+bwd")}
    peak = {}
    try:
        for u in (False, True):  # warm both paths, and the peak memory of one forward + backward on each
            tr._ATTN_UNFUSED = u
            fwd_bwd()
            torch.cuda.synchronize()
            x.grad = None
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd()
            torch.cuda.synchronize()
            peak[u] = torch.cuda.max_memory_allocated() - base
        for _ in range(rounds):
            for u in (False, True):
                tr._ATTN_UNFUSED = u
                times[(u, "fwd")].append(timeit(fwd, iters, 1))
                times[(u, "fwd+bwd")].append(timeit(fwd_bwd, iters, 1))
    finally:
        tr._ATTN_UNFUSED = saved
    for u, name in ((False, "fused"), (True, "gemm ")):
        for n, f in (("fwd", fl), ("fwd+bwd", 3.5 * fl)):
            ts = times[(u, n)]
            med, lo = statistics.median(ts), min(ts)
            print(f"AttentionF {name} {n:8s} median {med:9.1f} us  min {lo:9.1f} us  ({f / med / 1e6:.0f} TFLOP/s at the median)")
        print(f"AttentionF {name} peak memory above the inputs, one fwd+bwd: {peak[u] / 1e6:.0f} MB")
    for n in ("fwd", "fwd+bwd"):
        r = statistics.median(times[(True, n)]) / statistics.median(times[(False, n)])
        print(f"gemm / fused, {n}: {r:.2f}x")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=197)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--unfused-too", action="store_true")
    a = ap.parse_args()
    B, T, H, D = a.B, a.T, a.H, 64
    torch.manual_seed(0)
    qkv = (torch.randn(B * T, 3 * H * D, device="cuda") * 0.5).bfloat16()
    scale = D ** -0.5
    fl = 4.0 * B * H * T * T * D
    if (T + 15) // 16 * 16 <= 256:
        p, out = C.attn_fwd_rows(qkv, B, T, H, scale)
        dout = torch.randn_like(out)
        t_f = timeit(lambda: C.attn_fwd_rows(qkv, B, T, H, scale))
        t_b = timeit(lambda: C.attn_bwd_rows(dout, qkv, p, B, T, H, scale))
        saved = f"P {p.numel() * 2 / 1e6:.0f} MB"
    else:  # key-blocked kernels: the log-sum-exp is saved, and the backward takes the forward's output
        lse, out = C.attn_fwd_rows(qkv, B, T, H, scale, True)
        dout = torch.randn_like(out)
        t_f = timeit(lambda: C.attn_fwd_rows(qkv, B, T, H, scale, True))
        t_b = timeit(lambda: C.attn_bwd_rows(dout, qkv, lse, B, T, H, scale, None, out))
        saved = f"lse {lse.numel() * 4 / 1e6:.1f} MB"
    print(f"attn fwd {t_f:.1f} us ({fl / t_f / 1e6:.0f} TFLOP/s), bwd {t_b:.1f} us ({2.5 * fl / t_b / 1e6:.0f} TFLOP/s), "
          f"{saved}")
    if a.unfused_too:
        unfused_too(qkv, dout, B, T, H, fl)


if __name__ == "__main__":
    main()
