"""Private builds of lib6dgs_hip.so with extra compiler flags, for A/B timing on the GPU box (loaded through SIXDGS_LIB):
    python tools/build_variant.py <name> [flags...]   ->  build/variants/lib_<name>.so
The sources and the base flags are build.py's.  build/ is git-ignored."""
import importlib.util, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("sixdgs_build", os.path.join(ROOT, "6dgs_amd", "build.py"))      # build.py alone: no torch
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)
name, flags = sys.argv[1], sys.argv[2:]
out = os.path.join(ROOT, "build", "variants", f"lib_{name}.so")
os.makedirs(os.path.dirname(out), exist_ok=True)
objs, procs = [], []
for f in build.SOURCES:
    o = os.path.join(ROOT, "build", "variants", f"{name}_{f[:-4]}.o")
    objs.append(o)
    procs.append(subprocess.Popen([build.HIPCC, *build.FLAGS, *flags, "-c", os.path.join(build.CSRC, f), "-o", o]))
for p in procs:
    if p.wait() != 0:
        raise SystemExit("hipcc failed")
subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", out])
for o in objs:
    os.remove(o)
print(out)
