"""Time the dropout kernels on ViT-B/16 training shapes (128 x 197 token rows): [25216, 768] and [25216, 3072] bf16.

Variants, alternated inside one process on the same tensors and repeated to show the spread:
  ringdp dropout_bf16      y = m * x                    against  torch.nn.functional.dropout(x)
  ringdp dropout_add_bf16  y = res + m * x              against  torch.nn.functional.dropout(x) + res
at p = 0.1.  Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.
The kernels are bandwidth-bound: the algorithm needs 4 B per element (read x, write y) and 6 B per element with the
residual; the table gives the achieved TB/s over those bytes and its share of the 6.29 TB/s measured float4-copy
bandwidth of an MI355X.  (The [25216, 768] tensors are 39 MB each and stay in the 256 MiB Infinity Cache between
launches, so that shape can exceed the HBM figure; the yardstick is ATen on the same tensors in the same process.)
The ringdp variants read a snapshot made once: the one-thread rng_tick launch a forward pays is timed on its own.

python tools/dropout_bench.py [--seconds 2] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import ringdp  # noqa: E402,F401
import ringdp.random as rr  # noqa: E402
from ringdp._native import C  # noqa: E402
from ringdp.ops.dropout import quantize_p  # noqa: E402

COPY_TBS = 6.29
SHAPES = [(25216, 768), (25216, 3072)]
P = 0.1


def make_variants(shape, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(shape, device=dev, generator=g).bfloat16()
    res = torch.randn(shape, device=dev, generator=g).bfloat16()
    snap = rr.Draw(dev).snapshot
    thr, _ = quantize_p(P)
    n = x.numel()
    tag = f"{shape[0]}x{shape[1]}"
    return [
        dict(name=f"ringdp dropout       {tag}", step=lambda: C.dropout_bf16(x, snap, 0, thr), bytes=4 * n),
        dict(name=f"torch  dropout       {tag}", step=lambda: F.dropout(x, P, True), bytes=4 * n),
        dict(name=f"ringdp dropout_add   {tag}", step=lambda: C.dropout_add_bf16(x, res, snap, 0, thr, 0, 0, 0),
             bytes=6 * n),
        dict(name=f"torch  dropout + add {tag}", step=lambda: F.dropout(x, P, True) + res, bytes=6 * n),
    ]


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
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropout_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rr.manual_seed(0, dev)
    vs = [v for shape in SHAPES for v in make_variants(shape, dev)]
    state = rr.state_tensor(dev)
    vs.append(dict(name="ringdp rng_tick (one per forward)", step=lambda: C.rng_tick(state), bytes=0))
    for v in vs:  # warm-up, then size the timed loop
        run(v["step"], 5)
        v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 20)) + 1)
        v["us"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["us"].append(1000.0 * run(v["step"], v["iters"]))
    print(f"p = {P}; bandwidth-bound, share of the {COPY_TBS} TB/s measured copy bandwidth")
    out = []
    for v in vs:
        best, worst = min(v["us"]), max(v["us"])
        tbs = v["bytes"] / (best * 1e-6) / 1e12
        print(f"{v['name']:<36} {' '.join(f'{u:8.2f}' for u in v['us'])} us  ({v['iters']} calls per repeat)  "
              f"best {tbs:.2f} TB/s = {100 * tbs / COPY_TBS:.0f}% of copy bandwidth  "
              f"spread {100 * (worst - best) / best:.1f}%")
        out.append(dict(name=" ".join(v["name"].split()), us=v["us"], iters=v["iters"], bytes=v["bytes"], tbs=tbs,
                        share_of_copy_bw=tbs / COPY_TBS))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(p=P, variants=out), f, indent=1)


if __name__ == "__main__":
    main()
