"""Build an A/B variant of the extension: one .hip source recompiled with extra -D flags, linked
with the current in-tree objects into variants/<name>.so (run with RINGDP_EXT_PATH=variants/<name>.so,
tools/gpu_ab_variants.sh).  usage: python tools/build_variant.py NAME csrc/kernels/x.hip -DFOO=1 ...

This is the only way to the diagnostic-build macros of the bf16 ConvNet kernels.  Each is read by one unit,
the source to give: FF in csrc/kernels/convnet_fwd.hip, C12 in convnet_bwd12.hip, C3 in convnet_bwd3.hip
(the stamp macro they share, convnet_device.h, expands in that unit).  They are the timing-only phase
ablations (wrong results) -DRINGDP_FF_ABLATE=n / -DRINGDP_C3_ABLATE=n / -DRINGDP_C12_ABLATE=n (bits at each
macro), the fused forward's phase stamps -DRINGDP_FF_STAMPS, those of the 8-wave conv3 dgrad role
-DRINGDP_C3_STAMPS and those of both roles of the 8-wave conv12 backward -DRINGDP_C12_STAMPS, e.g.
  python tools/build_variant.py c3_nowgrad csrc/kernels/convnet_bwd3.hip -DRINGDP_C3_ABLATE=4"""
import importlib.util
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("ringdp_build", ROOT / "ringdp" / "_build.py")
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)

name, src, defs = sys.argv[1], (ROOT / sys.argv[2]).resolve(), sys.argv[3:]
b.build(verbose=False)
out_dir = ROOT / __import__("os").environ.get("RINGDP_VARIANT_DIR", "variants")
out_dir.mkdir(exist_ok=True)
obj = out_dir / f"{name}.{src.stem}.o"
cmd = b._compile_cmd(src, obj)
cmd = cmd[:-4] + defs + cmd[-4:]
b._run(cmd)
hip, cpp = b._sources()
objs = [obj if s == src else b._obj_for(s) for s in hip + cpp]
b._run(b._link_cmd(objs, out_dir / f"{name}.so"))
print(out_dir / f"{name}.so")
