"""The kernel instances the library ships, read from the built gfx950 code objects (no GPU needed).

Every kernel template instance in csrc/inst_*.o and csrc/ntt_host.o (or, where the objects are not at hand, in the linked
library, which holds the same code objects) is listed by tools/check_spills.kernels_of, demangled and parsed into
(family, policy, template arguments).  tests/kernel_recipes.py maps every instance to a call that launches it;
tests/test_kernel_inventory.py checks that the map is complete, tests/test_gpu_kernel_instances.py runs it.
"""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")
LIB = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# template parameters after the policy, as the kernel templates declare them (ntt_kernels_*.h, host/*.inc)
FAMILIES = {
    "fused_kernel": ("LOGN", "INV", "KSH", "LASTINV", "LAZY", "MULTI"),
    "twophase_kernel": ("LEAD", "INV", "KSH"),
    "onepass_kernel": ("INV", "KSH", "MULTI"),
    "column_kernel": ("R", "INV", "KSH", "MULTI"),
    "team_kernel": ("LEAD", "INV", "KSH", "MULTI"),
    "fused_product_kernel": ("LOGN", "KSH", "ALAZY", "WHOLE", "MULTI", "BOTH", "PTRS"),
    "fused_product_small_kernel": ("LOGN", "KSH", "MULTI", "BOTH", "PTRS"),
    "team_product_kernel": ("LEAD", "KSH", "FOUR", "MULTI", "PTRS"),
    "dot_inv_kernel": ("LOGN", "KSH", "LASTINV", "MULTI", "PTRS"),
    "team_dot_kernel": ("LEAD", "KSH", "MULTI", "PTRS"),
    "fwd_mul_kernel": ("LOGN", "KSH", "MULTI", "PTRS"),
    "onepass_mul_kernel": ("KSH", "MULTI", "PTRS"),
    "team_mul_kernel": ("LEAD", "KSH", "MULTI", "PTRS"),
    # host layer (csrc/host/*.inc): templates over the policy and run-time forms
    "pointwise_kernel": ("LAZYIN",),
    "pointwise_acc_kernel": ("LAZYIN", "ACC"),
    "pointwise_ptrs_kernel": ("LAZYIN", "ACC", "BCAST"),
}
# kernels that are no template over a policy: plan setup, utilities, the reference-signature shims
PLAIN = ("team_ctl_clear_kernel", "r4x4_r4_layer_kernel", "r4x4_r2_layer_kernel", "rmw_probe_kernel", "copy_probe_kernel",
         "shape_probe_kernel", "power_table_kernel", "records_u64_kernel", "records_f64_kernel", "records_r4_kernel",
         "fill_uniform_kernel", "checksum_kernel")

Instance = collections.namedtuple("Instance", "key family policy args")  # args: dict parameter -> int / bool


def demangler():
    for exe in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if exe and os.path.exists(exe):
            return exe
    raise RuntimeError("no C++ demangler (llvm-cxxfilt, c++filt) on this machine")


def demangle(names):
    names = list(names)
    if not names:
        return []
    out = subprocess.run([demangler()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert len(lines) == len(names), "demangler output does not line up with its input"
    return lines


def _split_args(s):
    """top-level comma split of a template argument list"""
    parts, depth, cur = [], 0, ""
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur.strip())
    return parts


def normalise(demangled):
    """the canonical key of a demangled kernel name: 'family<policy,arg,...>' (no return type, namespace, parameters or
    spaces) -- the same for the names objects carry and the names a kernel trace reports"""
    s = demangled.strip()
    s = re.sub(r"^void\s+", "", s)
    s = re.sub(r"\s+", "", s)
    s = s.replace("ntt::", "").replace("(anonymousnamespace)::", "")
    # cut the parameter list: the first '(' at template depth 0
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.replace("WideF64<ArithF64>", "ArithF64W")


def parse(key):
    """Instance of a normalised key; family None when the name belongs to no known family"""
    m = re.match(r"^(\w+)(?:<(.*)>)?$", key)
    if not m:
        return Instance(key, None, None, {})
    fam, targs = m.group(1), m.group(2)
    if fam in PLAIN and targs is None:
        return Instance(key, fam, None, {})
    if fam not in FAMILIES or targs is None:
        return Instance(key, None, None, {})
    parts = _split_args(targs)
    names = FAMILIES[fam]
    if len(parts) != len(names) + 1:
        return Instance(key, None, None, {})
    args = {}
    for n, v in zip(names, parts[1:]):
        if v in ("true", "false"):
            args[n] = v == "true"
        elif re.match(r"^-?\d+$", v):
            args[n] = int(v)
        else:
            return Instance(key, None, None, {})
    return Instance(key, fam, parts[0], args)


def objects():
    objs = sorted(glob.glob(os.path.join(CSRC, "inst_*.o")))
    host = os.path.join(CSRC, "ntt_host.o")
    if objs and os.path.exists(host):
        return objs + [host]
    if os.path.exists(LIB):
        return [LIB]
    raise RuntimeError("no built objects under %s and no %s: build first (make lib)" % (CSRC, LIB))


_cache = {}


def instances():
    """{key: Instance} of every kernel the library ships (a static kernel that several translation units define once each,
    team_ctl_clear_kernel, is one entry)"""
    if "inv" not in _cache:
        import check_spills
        mangled = sorted({k["name"] for o in objects() for k in check_spills.kernels_of(o)})
        _cache["inv"] = {}
        for m, d in zip(mangled, demangle(mangled)):
            key = normalise(d)
            _cache["inv"][key] = parse(key)
    return _cache["inv"]


def case_id(inst):
    """a readable pytest id: family, policy and the arguments that are set"""
    if not inst.args:
        return inst.family or inst.key
    bits = []
    for n, v in inst.args.items():
        if isinstance(v, bool):
            if v:
                bits.append(n)
        else:
            bits.append("%s%d" % (n, v))
    return "%s-%s-%s" % (inst.family, inst.policy, "-".join(bits))


if __name__ == "__main__":
    inv = instances()
    by = collections.Counter(i.family for i in inv.values())
    for fam, n in sorted(by.items(), key=lambda x: str(x[0])):
        print("%-28s %5d" % (fam, n))
    print("total", len(inv))
