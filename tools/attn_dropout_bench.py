"""Time the attention kernels with dropout on the probabilities (csrc/kernels/vit_attn_drop.hip) against the
key-blocked kernels without dropout of the same tree (``force_long``: the same work split, no mask).

Shapes: B = 128, H = 12, head dim 64, T = 197 (ViT-B/16 at 224) and T = 577 (at 384), p = 0.1, bf16.  Forward and
backward calls are timed with device events after warm-up, the two variants of a shape alternated inside one process
and repeated to show the spread; a backward call is two kernels (query side, key side).  The table gives the ratio
to the no-dropout kernels and the MFMA TFLOP/s over the algorithm's operations (forward 4 B H T^2 64, backward 10 B H
T^2 64 with the recomputed S).  ``--step`` also times one ViT-B/16 training step (forward + backward + SGD, B = 128,
replayed from a hipGraph) with ``dropout=0.1`` alone and with ``attention_dropout=0.1`` on top, alternated.

python tools/attn_dropout_bench.py [--seconds 1] [--repeats 3] [--step] [--json out.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ringdp  # noqa: E402,F401
import ringdp.random as rr  # noqa: E402
from ringdp._native import C  # noqa: E402
from ringdp.ops.dropout import quantize_p8  # noqa: E402

B, H, P = 128, 12, 0.1
LENGTHS = [197, 577]
SCALE = 0.125


def make_variants(T, dev):
    g = torch.Generator(device=dev).manual_seed(T)
    qkv = (torch.randn(B * T, 3 * H * 64, device=dev, generator=g) * 0.5).bfloat16()
    dout = torch.randn(B * T, H * 64, device=dev, generator=g).bfloat16()
    snap = rr.Draw(dev).snapshot
    thr8, _ = quantize_p8(P)
    lse, out = C.attn_fwd_rows(qkv, B, T, H, SCALE, True, force_long=True)
    lse_d, out_d = C.attn_drop_fwd_rows(qkv, B, T, H, SCALE, snap, 0, thr8)
    flop = B * H * T * T * 64
    return [
        dict(name=f"fwd          T={T}", flop=4 * flop,
             step=lambda: C.attn_fwd_rows(qkv, B, T, H, SCALE, True, force_long=True)),
        dict(name=f"fwd  dropout T={T}", flop=4 * flop,
             step=lambda: C.attn_drop_fwd_rows(qkv, B, T, H, SCALE, snap, 0, thr8)),
        dict(name=f"bwd          T={T}", flop=10 * flop,
             step=lambda: C.attn_bwd_rows(dout, qkv, lse, B, T, H, SCALE, None, out, force_long=True)),
        dict(name=f"bwd  dropout T={T}", flop=10 * flop,
             step=lambda: C.attn_drop_bwd_rows(dout, qkv, lse_d, out_d, B, T, H, SCALE, snap, 0, thr8)),
    ]


def make_steps(dev):
    """One captured ViT-B/16 training step per configuration (bf16, B = 128)."""
    import torch.nn.functional as F
    from ringdp.models import vit_b_16
    from ringdp.optim import SGD
    from ringdp.utils.graph import StepGraph

    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
    y = torch.randint(0, 1000, (B,), device=dev, generator=g)
    vs = []
    for name, kw in (("step dropout=0.1", dict(dropout=0.1)),
                     ("step dropout=0.1 attention_dropout=0.1", dict(dropout=0.1, attention_dropout=P))):
        torch.manual_seed(0)
        model = vit_b_16(**kw).to(dev).train()
        opt = SGD(model.parameters(), lr=1e-3, momentum=0.9)

        def step_fn(model=model, opt=opt):
            loss = F.cross_entropy(model(x), y)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()
            return loss

        graph = StepGraph(step_fn, warmup=3).capture()
        vs.append(dict(name=name, flop=0, step=graph.replay))
    return vs


def run(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time one ViT-B/16 training step with and without")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_dropout_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rr.manual_seed(0, dev)
    vs = [v for T in LENGTHS for v in make_variants(T, dev)]
    if a.step:
        vs += make_steps(dev)
    for v in vs:  # warm-up, then size the timed loop
        run(v["step"], 5)
        v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 10)) + 1)
        v["us"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["us"].append(1000.0 * run(v["step"], v["iters"]))
    print(f"B = {B}, H = {H}, p = {P}; each dropout row against the row above it")
    out = []
    for i, v in enumerate(vs):
        best, worst = min(v["us"]), max(v["us"])
        ratio = best / min(vs[i - 1]["us"]) if i % 2 else 1.0
        tf = v["flop"] / (best * 1e-6) / 1e12
        print(f"{v['name']:<40} {' '.join(f'{u:9.1f}' for u in v['us'])} us  ({v['iters']} calls per repeat)  "
              f"{tf:6.1f} TFLOP/s  x{ratio:.3f}  spread {100 * (worst - best) / best:.1f}%")
        out.append(dict(name=" ".join(v["name"].split()), us=v["us"], iters=v["iters"], tflops=tf, ratio=ratio))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(B=B, H=H, p=P, variants=out), f, indent=1)


if __name__ == "__main__":
    main()
