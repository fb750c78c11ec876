"""CPU: the C-ABI library loads, exports every symbol the headers declare, and
fails loudly (no CPU fallback) when no HIP device is present.  No compute."""
import os
import re
import subprocess

import pytest

import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    for hdr in ("ntt_mi355x.h", "ntt_reference.h", "ntt_radix4.h", "ntt_radix4x4.h", "ntt_seal.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"#\s*define[^\n]*", "", text)
        names |= set(re.findall(r"NTT_(?:API|EXPORT)\s+[\w\s\*]*?\b(\w+)\s*\(", text))
    return names


def test_exports_match_headers(lib):
    declared = _declared_symbols()
    assert len(declared) >= 38
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert declared <= exported, declared - exported
    assert set(lib.EXPORTED_SYMBOLS) == declared
    # nothing of the oracle may be linked into the product
    assert not any(s.startswith("orc_") for s in exported)
    needed = subprocess.check_output(["readelf", "-d", lib.LIB_PATH], text=True)
    assert "libntt_oracle" not in needed and "libamdhip64" in needed


def test_mul_op_abi():
    """mul_op_t keeps the reference ABI: two __uint128_t, 32 bytes, 16-aligned"""
    src = '#include "fast_mul_operators.h"\n_Static_assert(sizeof(mul_op_t)==32 && _Alignof(mul_op_t)==16,"abi");int main(void){return 0;}\n'
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include", "internal"), "-x", "c", "-"], input=src, text=True, check=True)


def test_mul_op_by_value_through_ctypes(lib, tmp_path):
    """the ctypes MulOp reaches a C callee intact even behind seven integer arguments (the first six go in
    registers, the seventh on the stack: an 8-aligned struct copy would then land 8 bytes off)"""
    import ctypes as C
    src = tmp_path / "probe.c"
    src.write_text('#include "fast_mul_operators.h"\n'
                   "uint64_t probe(long a,long b,long c,long d,long e,long f,long g, mul_op_t m)"
                   "{(void)a;(void)b;(void)c;(void)d;(void)e;(void)f;"
                   " return (uint64_t)m.op + 3*(uint64_t)(m.op>>64) + 5*(uint64_t)m.con + 7*(uint64_t)(m.con>>64) + (uint64_t)g;}\n")
    so = tmp_path / "probe.so"
    children.gcc("-shared", "-fPIC", "-I" + os.path.join(ROOT, "include", "internal"), "-o", so, src)
    probe = C.CDLL(str(so)).probe
    probe.restype = C.c_uint64
    probe.argtypes = [C.c_long] * 7 + [lib.MulOp]
    assert C.sizeof(lib.MulOp) == 32 and C.alignment(lib.MulOp) == 16
    m = lib._mulop((13 << 64) | 11, (19 << 64) | 17)
    assert probe(1, 2, 3, 4, 5, 6, 100, m) == 11 + 3 * 13 + 5 * 17 + 7 * 19 + 100


def test_plan_create_rejects_composite_modulus(lib):
    """q = 65 = 5 * 13 passes the cheap tests (4 | q-1, 8^2 = -1 mod 65) but is not prime: N^(q-2) is not
    N^-1, the plan would scale by garbage.  Refused before any device is touched."""
    import ctypes as C
    h = C.c_void_p()
    rc = lib._lib.ntt_plan_create(C.byref(h), 0, 2, 65, 8, 0)
    assert rc == -1 and "prime" in lib.last_error()


def test_traffic_json_matches_bench():
    """roofline.traffic in the bench line is read from a committed PMC summary: the file must name the kernel
    and batch bench.py launches by default, otherwise bench.py reports null rather than a stale number"""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    with open(bench.TRAFFIC_JSON) as f:
        t = json.load(f)
    assert t["kernel"] == bench.kernel_name(2) and t["batch"] == bench.per_gpu_batch("weak", 1) and t["N"] == bench.N
    assert t["hbm_bytes_per_launch"] == 2 * 1024 * t["FETCH_SIZE_KB"] + 1024 * t["WRITE_SIZE_KB"]
    assert bench.measured_traffic(t["batch"], t["kernel"]) == t["hbm_bytes_per_launch"]
    assert bench.measured_traffic(t["batch"], "fused_kernel<ArithU64,14,fwd>") is None
    assert bench.measured_traffic(t["batch"] // 2, t["kernel"]) is None
    # no more than 2 % above the algorithmic bytes: anything else means re-reads crept in
    assert 1.0 <= t["hbm_bytes_per_launch"] / (t["batch"] * 16 * t["N"]) < 1.02
    # The evidence is tied to the BINARY (review r05 item 3): every committed counter summary names the sha256 of the library it was
    # taken on, all of them the same one, and that is the library this tree builds (`make lib` is reproducible: the shipped .so is
    # rebuilt byte for byte from a `git archive`).  A kernel change after the collection fails here until tools/collect_r06.sh has
    # run again on the new library.
    import glob
    import hashlib
    shas = set()
    for f in glob.glob(os.path.join(bench.TRAFFIC_DIR, "pmc_traffic*.json")):
        with open(f) as fh:
            shas.add(json.load(fh).get("lib_sha256"))
    with open(os.path.join(bench.TRAFFIC_DIR, "LIBRARY_SHA256")) as fh:
        shas.add(fh.read().split()[0])
    assert len(shas) == 1 and None not in shas, shas
    lib = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    assert os.path.exists(lib), "build the library first (python -c 'import __graft_entry__ as g; g.build()')"
    with open(lib, "rb") as fh:
        built = hashlib.sha256(fh.read()).hexdigest()
    assert built in shas, "profiles/r06 was collected on library %s, this tree builds %s: run tools/collect_r06.sh again" % (shas, built)
    assert bench.traffic_lib_sha256() == built


def test_headers_compile_as_c_and_cxx():
    for comp, std in (("gcc", "-std=gnu11"), ("g++", "-std=c++17")):
        src = "\n".join('#include "%s"' % h for h in ("ntt_mi355x.h", "ntt_reference.h", "ntt_radix4.h",
                                                      "ntt_radix4x4.h", "ntt_seal.h", "pre_compute.h")) + "\nint main(void){return 0;}\n"
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "internal"),
                        "-x", "c" if comp == "gcc" else "c++", "-"], input=src, text=True, check=True)


def test_host_table_builders_match_oracle(oracle, kat, tmp_path):
    """include/internal/pre_compute.h (the builders the reference's test_cases.h
    calls) produce the golden tables"""
    prog = tmp_path / "t.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stdlib.h>
#include "pre_compute.h"
static unsigned long long fnv(const uint64_t *a, size_t n){unsigned long long h=0xcbf29ce484222325ULL;
 for(size_t i=0;i<n;i++)for(int b=0;b<8;b++){h^=(a[i]>>(8*b))&0xff;h*=0x100000001b3ULL;}return h;}
int main(int argc,char**argv){uint64_t m=strtoull(argv[1],0,0),q=strtoull(argv[2],0,0),w=strtoull(argv[3],0,0),n=1ULL<<m;
 uint64_t *t=malloc(8*n),*c=malloc(8*n),*e=malloc(16*n),*ec=malloc(16*n);
 calc_w(t,w,n,q,m);calc_w_con(c,t,n,q,WORD_SIZE);expand_w(e,t,n,q);calc_w_con(ec,e,2*n,q,WORD_SIZE);
 printf("%016llx %016llx %016llx %016llx\n",fnv(t,n),fnv(c,n),fnv(e,2*n),fnv(ec,2*n));return 0;}
''')
    exe = tmp_path / "t"
    children.gcc("-I" + os.path.join(ROOT, "include", "internal"), "-o", exe, prog)
    for i in (0, 4, 12, 13, 18):
        c = kat["cases"][i]
        out = subprocess.check_output([str(exe), str(c["m"]), str(c["q"]), str(c["w"])], text=True).split()
        t = c["table_fnv"]
        assert out == [t["w"], t["wcon"], t["e"], t["econ"]]


def test_no_device_fails_loudly(lib):
    """On a machine without a GPU every compute entry point must refuse, never
    silently compute on the CPU.  (On the GPU box this test is vacuous.)"""
    try:
        n = lib.device_count()
    except lib.NttError:
        n = 0
    if n > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(lib.NttError) as e:
        lib.Plan(256, 0x1e01, 62)
    assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)


def test_parameter_helpers(lib, oracle, kat):
    for c in kat["cases"][:8]:
        assert lib.min_root(c["q"], 1 << c["m"]) == c["w"]
    assert lib.find_prime(50, 1 << 14) == oracle.find_prime(50, 1 << 14)
    assert lib.min_root(7, 16) == 0
    assert lib.min_root(0x3fffffffe8001, 1 << 12) == 0     # composite modulus: refused, not searched forever


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libntt_ref.so")),
                    reason="build() compiled no reference binaries into oracle/_ref: the reference sources were not there")
def test_reference_drivers_compile_unchanged_against_our_headers(lib):
    """SURVEY 8b 'drop in unchanged': the reference's own tests/main.c, test_correctness.c and bench.c, compiled by build()
    against include/ (oracle/Makefile `dropin`, beside oracle/_ref/libntt_ref.so), are linked to libntt_mi355x.so and take
    every function they call from it or from the C library."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for exe in ("ntt-variants-dropin", "ntt-variants-bench-dropin"):
        path = os.path.join(ROOT, "oracle", "_ref", exe)
        assert os.path.exists(path), exe
        assert "[libntt_mi355x.so]" in subprocess.check_output(["readelf", "-d", path], text=True), exe
        undef = [l.split() for l in subprocess.check_output(["nm", "-D", "--undefined-only", path], text=True).splitlines()]
        ours = {f[-1] for f in undef if f[0] == "U" and "@" not in f[-1]}      # (versioned names: the C library's)
        assert ours and ours <= exported, (exe, ours - exported)


@pytest.mark.parametrize("example", ["batched_product", "rns_chain_product", "pointer_batch", "rns_ciphertext_tensor"])
def test_c_example_builds_against_the_public_header(lib, example):
    """examples/*.c that need nothing but the public header: plain-C callers (gcc, no HIP headers) compile and link against
    include/ntt_mi355x.h + libntt_mi355x.so; the GPU suite runs them (test_c_example_*_runs)"""
    assert os.path.exists(children.build_example(lib, example, *children.STRICT))


def _last_template_bool_is_multi(name):
    """is this mangled kernel name a MULTI variant (several RNS limbs in one launch)?  Position of the MULTI argument:
    fused_kernel<A, LOGN, INV, KSH, LASTINV, LAZY, MULTI>, column_kernel<A, R, INV, KSH, MULTI>, team_kernel<A, LEAD, INV, KSH,
    MULTI>, team_product_kernel<A, LEAD, KSH, FOUR, MULTI>, dot_inv_kernel<A, LOGN, KSH, LASTINV, MULTI>: last;
    fused_product_kernel<A, LOGN, KSH, ALAZY, WHOLE, MULTI, BOTH>, fused_product_small_kernel<A, LOGN, KSH, MULTI, BOTH>: second to last"""
    import re
    head = name.split("EEEvNS_")[0] + "E"
    args = re.findall(r"(Lb[01]E|Li\d+E)", head)
    if "fused_product_small" in name:
        return len(args) >= 4 and args[-2] == "Lb1E"
    if "fused_product_kernel" in name:
        return len(args) >= 6 and args[-2] == "Lb1E"
    if "team_product_kernel" in name or "team_kernel" in name or "dot_inv_kernel" in name or "column_kernel" in name:
        return args[-1] == "Lb1E"
    if "fused_kernel" in name:
        return len(args) >= 6 and args[-1] == "Lb1E" and args[-3].startswith("Lb")
    return False


def test_headline_kernels_do_not_spill():
    """persistent kernels for blocks >= 2^12 must be scratch-free (a spill reload is a vmcnt(0) wait queued
    behind the HBM prefetch: measured -40 %); read from the built objects' metadata, no GPU needed"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_spills
    every = check_spills.all_kernels()
    # the MULTI variants (several RNS limbs in one launch: the limb's tables are picked at run time from an array in the
    # kernel arguments) spilled 2-6 VGPRs in rounds 3 and 4 -- not because of the run-time index but because the limb came out
    # of a VALU division and dragged every address after it into vector registers; since round 5 (the limb is blockIdx.y, the
    # queue kernels split with a scalar multiply-high: csrc/ntt_kernels_block.h limb_params, ntt_kernels_team.h team_split) they are held to the same rule
    multi = [k for k in every if _last_template_bool_is_multi(k["name"])]
    ks = [k for k in every if k not in multi]
    assert len(ks) >= 80 and len(multi) >= 40
    for k in multi:
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    fused = [k for k in ks if "fused_kernel" in k["name"] and "ArithF64" in k["name"]]
    big = [k for k in fused if any(("ELi%dE" % ln) in k["name"] for ln in (12, 13, 14))]
    # 3 block sizes x (3 headroom classes + the wide policy for q up to 2^52) x {fwd, fwd with lazy outputs, inv},
    # + per class the 2^14 and 2^12 inverses that do not end a transform (blocks below a column pass)
    assert len(big) == 3 * 4 * 3 + 4 + 4
    for k in big:
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    # (rounds 2-4 had one exception, the one-launch product at 2^14 for 52-bit moduli: its two spilled VGPRs were the block count,
    # copied into vector registers for a 64-bit unsigned comparison that has no scalar form -- csrc/ntt_kernels_block.h `below`)
    for k in ks:
        assert k["group_segment_fixed_size"] <= 160 * 1024, k
        assert k["vgpr_spill_count"] == 0, k   # no kernel of the library spills vector registers
