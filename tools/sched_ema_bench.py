"""Time one ModelEma.update() over the parameter list of ringdp.models.vit_b_16 (about 86 M fp32 parameters), and one
device-side scheduler step.

Variants, alternated inside one process and repeated to show the spread:
  ringdp ModelEma.update(), multi-tensor (separate parameter tensors) and flat (the parameters are views of one
  flattened buffer, as ringdp's DDP lays them out);
  torch._foreach_lerp_(shadows, params, w) with a host-side weight, which is what timm's ModelEmaV2 runs;
  ringdp WarmupCosineLR.step() over 2 parameter groups (one launch of one workgroup).
Timed with device events after warm-up, at least ``--seconds`` of timed work per variant and repeat.  The update is
bandwidth-bound: the algorithm needs 12 B per element (read p and e, write e); the table gives the achieved TB/s over
those bytes and its share of the 6.29 TB/s measured float4-copy bandwidth of an MI355X (the figure
tools/dropout_bench.py and tools/optim_bench.py use).

python tools/sched_ema_bench.py [--seconds 2] [--repeats 3] [--json out.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ringdp  # noqa: E402
from ringdp.models import vit_b_16  # noqa: E402
from ringdp.utils import ModelEma  # noqa: E402

COPY_TBS = 6.29


class Bag(torch.nn.Module):
    def __init__(self, shapes, dev, flat):
        super().__init__()
        torch.manual_seed(3)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, device=dev).mul_(0.02)) for s in shapes])
        if flat:  # the layout DistributedDataParallel installs: views of one buffer, _ringdp_flat on each parameter
            offs, tot = [], 0
            for p in self.ps:
                offs.append(tot)
                tot += (p.numel() + 15) // 16 * 16
            fp, fg = torch.zeros(tot, device=dev), torch.zeros(tot, device=dev)
            for p, o in zip(self.ps, offs):
                view = fp[o:o + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p._ringdp_flat = (fp, fg, o, len(self.ps))


def make_variants(shapes, dev):
    multi, flat = Bag(shapes, dev, False), Bag(shapes, dev, True)
    ema_m, ema_f = ModelEma(multi, decay=0.9999), ModelEma(flat, decay=0.9999)
    ref = Bag(shapes, dev, False)
    shadows = [p.detach().clone() for p in ref.ps]
    params = [p.detach() for p in ref.ps]
    groups = [dict(params=[torch.zeros(8, device=dev, requires_grad=True)], lr=lr) for lr in (1e-3, 1e-4)]
    sched = ringdp.optim.lr_scheduler.WarmupCosineLR(ringdp.optim.AdamW(groups), 10 ** 9, warmup_steps=10 ** 4)
    n = sum(p.numel() for p in multi.ps)
    return [
        dict(name="ringdp ModelEma.update multi", step=ema_m.update, bytes=12 * n, keep=(multi, ema_m)),
        dict(name="ringdp ModelEma.update flat", step=ema_f.update, bytes=12 * n, keep=(flat, ema_f)),
        dict(name="torch  _foreach_lerp_", step=lambda: torch._foreach_lerp_(shadows, params, 1e-4), bytes=12 * n),
        dict(name="ringdp WarmupCosineLR.step", step=sched.step, bytes=0, keep=sched),
    ], n


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
        raise SystemExit("sched_ema_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    shapes = [tuple(p.shape) for p in vit_b_16().parameters()]
    vs, n = make_variants(shapes, dev)
    for v in vs:  # warm-up (builds the tables), then size the timed loop
        run(v["step"], 5)
        v["iters"] = max(10, int(a.seconds * 1000.0 / run(v["step"], 20)) + 1)
        v["us"] = []
    for _ in range(a.repeats):
        for v in vs:
            v["us"].append(1000.0 * run(v["step"], v["iters"]))
    print(f"{len(shapes)} tensors, {n} elements ({n * 4 / 1e6:.0f} MB of fp32 parameters); bandwidth-bound, "
          f"share of the {COPY_TBS} TB/s measured copy bandwidth")
    out = []
    for v in vs:
        best, worst = min(v["us"]), max(v["us"])
        tbs = v["bytes"] / (best * 1e-6) / 1e12
        print(f"{v['name']:<30} {' '.join(f'{u:9.2f}' for u in v['us'])} us  ({v['iters']} calls per repeat)  "
              f"best {tbs:.2f} TB/s = {100 * tbs / COPY_TBS:.0f}% of copy bandwidth  "
              f"spread {100 * (worst - best) / best:.1f}%")
        out.append(dict(name=" ".join(v["name"].split()), us=v["us"], iters=v["iters"], bytes=v["bytes"], tbs=tbs,
                        share_of_copy_bw=tbs / COPY_TBS))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(elements=n, tensors=len(shapes), variants=out), f, indent=1)


if __name__ == "__main__":
    main()
