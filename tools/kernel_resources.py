"""Print register / LDS / spill figures of the kernels of one HIP source (cross-compiles to gfx950 assembly).

python tools/kernel_resources.py [SRC] [NAME_FILTER] [--digest]

--digest also prints a hash of each kernel's instruction stream and its sgpr count and scratch size, full names
and nothing else per line: two trees whose digests diff clean compile every kernel to the same code."""
import hashlib, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
digest = "--digest" in sys.argv
args = [a for a in sys.argv[1:] if a != "--digest"]
src = args[0] if args else os.path.join(ROOT, "6dgs_amd", "csrc", "score.hip")
flt = args[1] if len(args) > 1 else ""
out = os.path.join(ROOT, "gpurun_out", "asm")
os.makedirs(out, exist_ok=True)
asm = os.path.join(out, os.path.basename(src) + ".s")
subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", *os.environ.get("SIXDGS_EXTRA_FLAGS", "").split(), "-S", "--cuda-device-only",
                       "-o", asm, src], stderr=subprocess.DEVNULL)
t = open(asm).read()
g = lambda blk, k: re.search(r"\." + k + r":\s+(\d+)", blk).group(1)


def code_hash(nm):
    """The kernel's instructions from its entry label to its descriptor, comments stripped and the block labels'
    function number (.LBB<n>_) dropped: adding or removing a kernel renumbers the labels of the ones after it."""
    body = re.search(r"^" + re.escape(nm) + r":[^\n]*\n(.*?)^\s*\.section\s+\.rodata", t, re.S | re.M).group(1)
    body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";[^\n]*", "", body))
    return hashlib.sha256("\n".join(ln.strip() for ln in body.splitlines() if ln.strip()).encode()).hexdigest()[:16]


if digest:
    print("kernel code_hash agpr vgpr(total) lds sgpr_spill vgpr_spill sgpr scratch")
else:
    print(f"{'kernel':70s} agpr vgpr(total)  lds  sgpr_spill vgpr_spill")
for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size", t, re.S):
    blk = m.group(0)
    nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
    if flt not in nm:
        continue
    if digest:
        print(nm, code_hash(nm), *(g(blk, k) for k in ("agpr_count", "vgpr_count", "group_segment_fixed_size", "sgpr_spill_count",
                                                     "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size")))
    else:
        print(f"{nm[:70]:70s} {g(blk,'agpr_count'):>4s} {g(blk,'vgpr_count'):>6s} {g(blk,'group_segment_fixed_size'):>8s} {g(blk,'sgpr_spill_count'):>6s} {g(blk,'vgpr_spill_count'):>6s}")
