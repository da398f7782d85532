"""Time one optimizer step over the parameter list of ringdp.models.vit_b_16 (about 86 M fp32 parameters).

Variants, alternated inside one process and repeated to show the spread:
  ringdp AdamW (multi-tensor), without clipping and with max_grad_norm=1.0;
  torch.optim.AdamW(fused=True) and (foreach=True), alone and preceded by torch.nn.utils.clip_grad_norm_.
Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.  The step is
bandwidth-bound: the algorithm needs 28 B per element for the update (read p, g, m, v; write p, m, v) plus 4 B per
element for the norm pass; the table gives the achieved TB/s over those bytes and its share of the 6.29 TB/s
measured float4-copy bandwidth of an MI355X.

python tools/optim_bench.py [--seconds 2] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ringdp  # noqa: E402
from ringdp.models import vit_b_16  # noqa: E402

COPY_TBS = 6.29


def make_variant(name, shapes, dev):
    torch.manual_seed(3)
    ps = [torch.randn(s, device=dev).mul_(0.02).requires_grad_() for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev)
    kw = dict(lr=1e-3, weight_decay=1e-2)
    clip = name.endswith("+clip")
    if name.startswith("ringdp"):
        opt = ringdp.optim.AdamW(ps, max_grad_norm=1.0 if clip else None, **kw)
        step = opt.step
    else:
        opt = torch.optim.AdamW(ps, fused=True, **kw) if "fused" in name else torch.optim.AdamW(ps, foreach=True, **kw)
        if clip:
            def step():
                torch.nn.utils.clip_grad_norm_(ps, 1.0)
                opt.step()
        else:
            step = opt.step
    return dict(name=name, step=step, clip=clip, keep=(ps, opt))


def run(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms per step


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = [tuple(p.shape) for p in vit_b_16().parameters()]
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    names = ["ringdp", "ringdp+clip", "torch-fused", "torch-foreach", "torch-fused+clip", "torch-foreach+clip"]
    vs = [make_variant(nm, shapes, dev) for nm in names]
    for v in vs:  # warm-up (builds tables and state), then size the timed loop
        run(v["step"], 5)
        v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 20)) + 1)
        v["ms"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["ms"].append(run(v["step"], v["iters"]))
    print(f"{len(shapes)} tensors, {n} elements ({n * 4 / 1e6:.0f} MB of fp32 parameters); bandwidth-bound, "
          f"share of the {COPY_TBS} TB/s measured copy bandwidth")
    out = []
    for v in vs:
        nbytes = n * (28 + (4 if v["clip"] else 0))
        best, worst = min(v["ms"]), max(v["ms"])
        tbs = nbytes / (best * 1e-3) / 1e12
        print(f"{v['name']:<20} {' '.join(f'{m:8.4f}' for m in v['ms'])} ms/step  ({v['iters']} steps per repeat)  "
              f"needs {nbytes / 1e9:.3f} GB  best {tbs:.2f} TB/s = {100 * tbs / COPY_TBS:.0f}% of copy bandwidth  "
              f"spread {100 * (worst - best) / best:.1f}%")
        out.append(dict(name=v["name"], ms=v["ms"], iters=v["iters"], bytes=nbytes, tbs=tbs,
                        share_of_copy_bw=tbs / COPY_TBS))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(elements=n, tensors=len(shapes), variants=out), f, indent=1)


if __name__ == "__main__":
    main()
