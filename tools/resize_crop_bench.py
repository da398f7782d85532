"""Time the device loader's random-resized-crop path at ViT fine-tuning shapes: B = 128 samples of a CIFAR-shaped
uint8 dataset (32 x 32 x 3, HBM-resident) to S = 224 and 384, bf16, NCHW.

Variants, alternated inside one process on the same tensors and repeated to show the spread, per S:
    ringdp rng_tick + crop_draw + resize_crop   what ``DeviceLoader(resize=S).batch()`` launches
    ringdp resize_crop alone                    records made once
    ATen per-sample                             slice, F.interpolate, flip, normalise, cast, per sample (boxes and
                                                flips read to the host once, outside the timed loop), then a stack
    ATen copy of the output                     ``torch.empty_like(out).copy_(out)``: the store-bandwidth yardstick
Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.  The kernel reads
3 KiB per sample and writes ``B * 3 * S * S`` bf16 values, so the output bytes are the algorithm's bytes; the table
gives the achieved TB/s over them and the time as a multiple of the copy's (which reads as much as it writes).

python tools/resize_crop_bench.py [--seconds 2] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import ringdp  # noqa: E402,F401
import ringdp.random as rr  # noqa: E402
from ringdp._native import C  # noqa: E402
from ringdp.data import DeviceLoader, SyntheticImages  # noqa: E402

BATCH = 128
SOURCE = (32, 32, 3)
SIZES = (224, 384)
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def variants(dev, S):
    ds = SyntheticImages(4096, SOURCE, 10, seed=1)
    loader = DeviceLoader(ds, BATCH, dev, hflip=True, mean=MEAN, std=STD, out_dtype=torch.bfloat16, resize=S)
    idx = torch.randperm(4096, generator=torch.Generator().manual_seed(2))[:BATCH].to(dev)
    rec = C.crop_draw(rr.Draw(dev).snapshot, BATCH, SOURCE[0], SOURCE[1], S, loader.crop_scale, *loader.draw_cfg)
    out, _ = loader.batch(idx, 0)
    boxes = rec.cpu().tolist()
    rows = idx.cpu().tolist()
    x = loader.x
    mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    inv_std = 1.0 / torch.tensor(STD, device=dev).view(1, 3, 1, 1)

    def aten():
        parts = []
        for i, (y0, x0, h, w, flip, *_rest) in zip(rows, boxes):
            crop = x[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].float()
            t = F.interpolate(crop, (S, S), mode="bilinear", align_corners=False)
            t = ((t.flip(3) if flip else t) / 255.0 - mean) * inv_std
            parts.append(t.to(torch.bfloat16))
        return torch.cat(parts)

    nbytes = out.numel() * out.element_size()
    return [
        dict(name=f"S={S} ringdp tick + draw + resize_crop", step=lambda: loader.batch(idx, 0), bytes=nbytes),
        dict(name=f"S={S} ringdp resize_crop alone",
             step=lambda: C.resize_crop(x, loader.y, idx, rec, S, loader.mean, loader.std, False, torch.bfloat16),
             bytes=nbytes),
        dict(name=f"S={S} ATen per-sample crop + interpolate", step=aten, bytes=nbytes),
        dict(name=f"S={S} ATen copy of the output", step=lambda: torch.empty_like(out).copy_(out), bytes=nbytes),
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
        raise SystemExit("resize_crop_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rr.manual_seed(0, dev)
    vs = [v for S in SIZES for v in variants(dev, S)]
    for v in vs:  # warm-up, then size the timed loop
        run(v["step"], 3)
        v["iters"] = max(5, int(a.seconds * 1000.0 / run(v["step"], 5)) + 1)
        v["us"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["us"].append(1000.0 * run(v["step"], v["iters"]))
    out = []
    for k, v in enumerate(vs):
        best, worst = min(v["us"]), max(v["us"])
        copy = min(vs[k - k % 4 + 3]["us"])  # the copy of the same S
        tbs = v["bytes"] / (best * 1e-6) / 1e12
        print(f"{v['name']:<44} {' '.join(f'{u:9.2f}' for u in v['us'])} us  ({v['iters']} calls per repeat)  "
              f"best {tbs:.3f} TB/s written  {best / copy:7.2f} x the copy  spread {100 * (worst - best) / best:.1f}%")
        out.append(dict(name=v["name"], us=v["us"], iters=v["iters"], bytes=v["bytes"], tbs_written=tbs,
                        times_copy=best / copy))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(batch=BATCH, source=SOURCE, sizes=SIZES, variants=out), f, indent=1)


if __name__ == "__main__":
    main()
