"""Time the depthwise 7 x 7 convolution kernels on the four ConvNeXt-T stage shapes at batch 128 (NHWC bf16):
56^2 x 96, 28^2 x 192, 14^2 x 384, 7^2 x 768.

Variants, alternated inside one process on the same tensors and repeated to show the spread:
  ringdp dwconv_fwd (forward), dwconv_fwd(flip) (data gradient), dwconv_wgrad (weight + bias gradient, both launches)
against ATen on channels-last bf16 tensors with bf16 weights (what autocast runs): F.conv2d(groups=C),
torch.ops.aten.convolution_backward with only the input / only the weight + bias gradient asked for.
Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.  The kernels are
bandwidth-bound: forward and data gradient must read and write the activation once (4 B per element), the weight
gradient must read x and dy (4 B per element); the table gives the achieved TB/s over those bytes.

python tools/dwconv_bench.py [--seconds 1] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import ringdp  # noqa: E402,F401
from ringdp._native import C  # noqa: E402

SHAPES = [(128, 56, 56, 96), (128, 28, 28, 192), (128, 14, 14, 384), (128, 7, 7, 768)]
K = 7


def make_variants(shape, dev):
    N, H, W, Cc = shape
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(shape, device=dev, generator=g).bfloat16()
    dy = torch.randn(shape, device=dev, generator=g).bfloat16()
    w = torch.randn(Cc, 1, K, K, device=dev, generator=g) * 0.1
    b = torch.randn(Cc, device=dev, generator=g)
    xa, dya = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # NCHW views of channels-last memory
    wa, ba = w.bfloat16(), b.bfloat16()
    P = K // 2

    def aten_bwd(mask):
        return torch.ops.aten.convolution_backward(dya, xa, wa, [Cc], [1, 1], [P, P], [1, 1], False, [0, 0], Cc, mask)

    nbytes = 4 * x.numel()
    tag = f"{H}x{W}x{Cc}"
    return [
        dict(name=f"ringdp fwd   {tag}", step=lambda: C.dwconv_fwd(x, w, b, False), bytes=nbytes),
        dict(name=f"aten   fwd   {tag}", step=lambda: F.conv2d(xa, wa, ba, padding=P, groups=Cc), bytes=nbytes),
        dict(name=f"ringdp dgrad {tag}", step=lambda: C.dwconv_fwd(dy, w, None, True), bytes=nbytes),
        dict(name=f"aten   dgrad {tag}", step=lambda: aten_bwd([True, False, False]), bytes=nbytes),
        dict(name=f"ringdp wgrad {tag}", step=lambda: C.dwconv_wgrad(x, dy, K, True), bytes=nbytes),
        dict(name=f"aten   wgrad {tag}", step=lambda: aten_bwd([False, True, True]), bytes=nbytes),
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
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    out = []
    for shape in SHAPES:  # one shape at a time: its tensors are freed before the next
        vs = make_variants(shape, dev)
        for v in vs:  # warm-up, then size the timed loop
            run(v["step"], 5)
            v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 20)) + 1)
            v["us"] = []
        for _ in range(a.repeats):
            for v in vs:
                v["us"].append(1000.0 * run(v["step"], v["iters"]))
        for v in vs:
            best, worst = min(v["us"]), max(v["us"])
            tbs = v["bytes"] / (best * 1e-6) / 1e12
            print(f"{v['name']:<28} {' '.join(f'{u:9.2f}' for u in v['us'])} us  ({v['iters']} calls per repeat)  "
                  f"best {tbs:.2f} TB/s  spread {100 * (worst - best) / best:.1f}%", flush=True)
            out.append(dict(name=" ".join(v["name"].split()), us=v["us"], iters=v["iters"], bytes=v["bytes"],
                            tbs=tbs))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(K=K, variants=out), f, indent=1)


if __name__ == "__main__":
    main()
