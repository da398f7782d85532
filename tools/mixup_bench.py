"""Time Mixup / CutMix and the mixed-target cross entropy at DeiT training shapes.

Variants, alternated inside one process on the same tensors and repeated to show the spread:
  images [128, 3, 224, 224] bf16
    ringdp mix_draw + mix_images (mixup record)   against  x * lam + x.flip(0) * (1 - lam)   (ATen, lam a device scalar)
    ringdp mix_draw + mix_images (cutmix record)  against  the same ATen composition (ATen has no one-pass cutmix)
    ringdp mix_images alone, mixup / cutmix / not applied
  loss [128, 1000] fp32, forward + backward, through autograd and as the two ops alone
    ringdp mixed-target cross entropy (lam read from the records)  against  ringdp index-target cross entropy
Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.  The mix is
bandwidth-bound: mixup reads x twice and writes once (3 tensor sizes, 6 B per bf16 element), cutmix and the
not-applied copy read each output element's source once (4 B per element).  The ATen composition moves at least 5
tensor sizes (7 as three passes: each product reads and writes one, the sum reads two and writes one) but is charged
the algorithm's 6 B per element too.  The table gives the achieved TB/s over those bytes
and its share of the 6.29 TB/s measured float4-copy bandwidth of an MI355X.  (One image tensor is 38.5 MB and stays in the 256 MiB Infinity Cache between launches, so the
figures can exceed the HBM rate; the yardstick is ATen on the same tensors in the same process.)
The ringdp variants read a snapshot made once: the one-thread rng_tick launch is timed by tools/dropout_bench.py.

python tools/mixup_bench.py [--seconds 2] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ringdp  # noqa: E402,F401
import ringdp.random as rr  # noqa: E402
from ringdp._native import C  # noqa: E402
from ringdp.ops.loss import _CrossEntropy  # noqa: E402
from ringdp.ops.mixup import MixedTarget, lam_of, mixed_cross_entropy  # noqa: E402

COPY_TBS = 6.29
IMAGES = (128, 3, 224, 224)
LOGITS = (128, 1000)


def image_variants(dev):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(IMAGES, device=dev, generator=g).bfloat16()
    y = torch.randint(0, 1000, (IMAGES[0],), device=dev, generator=g)
    snap = rr.Draw(dev).snapshot
    H, W = IMAGES[2:]
    n = x.numel()
    recs = dict(mixup=C.mix_draw(snap, 1, H, W, 0.8, 0.0, 1.0, 0.5), cutmix=C.mix_draw(snap, 1, H, W, 0.0, 1.0, 1.0, 0.5),
                none=C.mix_draw(snap, 1, H, W, 0.8, 1.0, 0.0, 0.5))
    lam = lam_of(recs["mixup"]).to(torch.bfloat16).reshape(())
    rest = (1 - lam_of(recs["mixup"])).to(torch.bfloat16).reshape(())

    def pair(ma, ca):
        return C.mix_images(x, y, C.mix_draw(snap, 1, H, W, ma, ca, 1.0, 0.5))

    return [
        dict(name="ringdp draw + mix, mixup", step=lambda: pair(0.8, 0.0), bytes=6 * n),
        dict(name="ringdp draw + mix, cutmix", step=lambda: pair(0.0, 1.0), bytes=4 * n),
        dict(name="torch  x*lam + x.flip(0)*(1-lam)", step=lambda: x * lam + x.flip(0) * rest, bytes=6 * n),
        dict(name="ringdp mix_images, mixup", step=lambda: C.mix_images(x, y, recs["mixup"]), bytes=6 * n),
        dict(name="ringdp mix_images, cutmix", step=lambda: C.mix_images(x, y, recs["cutmix"]), bytes=4 * n),
        dict(name="ringdp mix_images, not applied", step=lambda: C.mix_images(x, y, recs["none"]), bytes=4 * n),
        dict(name="ringdp mix_draw alone", step=lambda: C.mix_draw(snap, 1, H, W, 0.8, 1.0, 1.0, 0.5), bytes=0),
    ]


def loss_variants(dev):
    g = torch.Generator(device=dev).manual_seed(4)
    logits = torch.randn(LOGITS, device=dev, generator=g).requires_grad_()
    y_a = torch.randint(0, LOGITS[1], (LOGITS[0],), device=dev, generator=g)
    rec = C.mix_draw(rr.Draw(dev).snapshot, LOGITS[0], 224, 224, 0.8, 1.0, 1.0, 0.5)
    target = MixedTarget(y_a, y_a.flip(0), lam_of(rec))
    n = logits.numel()

    def mixed():
        mixed_cross_entropy(logits, target, 0.1, "mean").backward()

    def index():
        _CrossEntropy.apply(logits, y_a, -100, 0.1, "mean").backward()

    # the algorithm's bytes: the forward reads the logits, the backward reads them again and writes the gradient
    # (512 KB of logits: these calls are bound by launch latency and autograd, not by bandwidth)
    z, y_b, lam, g = logits.detach(), y_a.flip(0), lam_of(rec), torch.ones((), device=dev)

    def mixed_ops():  # the two launches without autograd
        _, lse, ws = C.cross_entropy_mix_fwd(z, y_a, y_b, lam, 0.1, 1)
        C.cross_entropy_mix_bwd(z, y_a, y_b, lam, lse, ws, g, 0.1, 1)

    def index_ops():
        _, lse, ws = C.cross_entropy_fwd(z, y_a, -100, 0.1, 1)
        C.cross_entropy_bwd(z, y_a, lse, ws, g, -100, 0.1, 1)

    return [dict(name="ringdp mixed-target CE fwd + bwd", step=mixed, bytes=12 * n),
            dict(name="ringdp index-target CE fwd + bwd", step=index, bytes=12 * n),
            dict(name="ringdp mixed-target CE, ops only", step=mixed_ops, bytes=12 * n),
            dict(name="ringdp index-target CE, ops only", step=index_ops, bytes=12 * n)]


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
        raise SystemExit("mixup_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rr.manual_seed(0, dev)
    vs = image_variants(dev) + loss_variants(dev)
    for v in vs:  # warm-up, then size the timed loop
        run(v["step"], 5)
        v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 20)) + 1)
        v["us"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["us"].append(1000.0 * run(v["step"], v["iters"]))
    print(f"share of the {COPY_TBS} TB/s measured copy bandwidth over the algorithm's bytes")
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
            json.dump(dict(images=IMAGES, logits=LOGITS, variants=out), f, indent=1)


if __name__ == "__main__":
    main()
