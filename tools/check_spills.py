#!/usr/bin/env python3
"""Read register/scratch metadata of every gfx950 kernel in the built objects (no GPU needed).

A single spilled VGPR in the persistent NTT kernels costs ~40 % (its reload is an s_waitcnt vmcnt(0) queued
behind the HBM prefetch), so tests/test_abi.py asserts the headline kernels are spill-free.
usage: tools/check_spills.py [obj ...]   -> one line per kernel: name vgprs spills scratch lds"""
import glob, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels_of(obj):
    """kernels of an object file -- or of a linked library, whose .hip_fatbin holds one bundle per translation unit"""
    out = []
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        with open(fat, "rb") as f:
            blob = f.read()
        starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
        if not starts:
            raise RuntimeError("%s: no uncompressed offload bundle in .hip_fatbin (%d bytes)" % (obj, len(blob)))
        for i, s in enumerate(starts):
            one, co = os.path.join(d, "one.bin"), os.path.join(d, "dev.co")
            with open(one, "wb") as f:
                f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + one, "--output=" + co],
                                  stderr=subprocess.DEVNULL)
            out += _kernels_of_notes(subprocess.check_output([LLVM + "/llvm-readelf", "--notes", co], text=True))
    return out


def _kernels_of_notes(txt):
    # amdhsa.kernels is a YAML list; every kernel entry starts with "  - .<first key>:" (keys are sorted, so
    # .group_segment_fixed_size precedes .name inside one entry)
    out, cur = [], None
    in_kernels = False
    for line in txt.splitlines():
        if line.strip().startswith("amdhsa.kernels:"):
            in_kernels = True
            continue
        if not in_kernels:
            continue
        if re.match(r"^\S", line) and not line.startswith(" "):
            in_kernels = line.strip().startswith("amdhsa.kernels")
        m = re.match(r"^(\s*)(-\s+)?\.(\w+):\s*(.*)$", line)
        if not m: continue
        indent, dash, k, v = len(m.group(1)), m.group(2), m.group(3), m.group(4).strip()
        if dash and indent <= 2:
            cur = {}; out.append(cur)
        if cur is None or indent > 4: continue
        if k == "name": cur["name"] = v
        elif k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                   "group_segment_fixed_size", "agpr_count", "sgpr_count"):
            try: cur[k] = int(v)
            except ValueError: pass
    return [k for k in out if "name" in k and "vgpr_count" in k]


def all_kernels(objs=None):
    objs = objs or sorted(glob.glob(os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc", "inst_*.o")))
    res = []
    for o in objs:
        for k in kernels_of(o):
            k["obj"] = os.path.basename(o); res.append(k)
    return res


if __name__ == "__main__":
    for k in all_kernels(sys.argv[1:] or None):
        print("%-90s vgpr %3d spill %3d scratch %4d lds %6d" % (k["name"][:90], k.get("vgpr_count", -1), k.get("vgpr_spill_count", -1),
                                                               k.get("private_segment_fixed_size", -1), k.get("group_segment_fixed_size", -1)))
