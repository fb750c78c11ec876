"""CPU: the BGV ModDown (ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch) without a GPU -- the model of tests/bgv_model.py
against plain big-integer arithmetic (the result is y - v T with 0 <= v < np), its relation to the approximate ModDown at T = 1, the edge
words, a toy BGV multiplication that decrypts (and picks up q_L^-1 mod T at the modulus switch), the host side of csrc/ntt_bgv.h under
the address and undefined-behaviour sanitizers against 128-bit integers and the model (tests/bgv_host_check.cpp), the exported symbols
with their signatures, the option, the plain-C example against the public header alone and the kernels of the new translation units."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import bgv_model as bm
import children
import keyswitch_model as km
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd")
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
T = bm.TRANSFORMED
N = 64
PT = bm.PT


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_model_is_y_minus_v_t_against_big_integers(oracle, np_):
    """3 x 50-bit kept primes, np 60-bit P primes, T = 65537, 2000 random x in [0, QP): every limb holds (y - v T) mod q_l for ONE
    0 <= v < np; np = 1: only v = 0; np = 2, 4: every v occurs"""
    primes, roots = rs.chain(oracle, N, [50] * 3 + [60] * np_)
    nq, qp, pr = 3, primes[:3], primes[3:]
    Q = km.prod(qp)
    rng = random.Random(100 + np_)
    xs = [rng.randrange(Q * km.prod(pr)) for _ in range(2000)]
    got, t = bm.mod_down_bgv(oracle, primes, roots, np_, km.residues(xs, primes), len(xs), PT, 0)
    for j in range(np_):
        assert np.array_equal(t[j], km.residues(xs, pr)[j])
    seen = set()
    for x, r in zip(xs, km.crt(got, qp)):
        y, w = bm.definition(x, pr, PT)
        assert y % PT == x * pow(km.prod(pr), -1, PT) % PT, "y = x P^-1 mod T"
        d = (y - r) % Q
        assert d % PT == 0 and 0 <= d // PT < np_, (x, d)
        seen.add(d // PT)
    assert seen == set(range(np_)), seen


@pytest.mark.parametrize("qbits,pbits", [([50] * 5, [60, 60]), ([50] * 4, [50, 50, 50]), ([60] * 3, [60] * 8), ([50, 52], [60])],
                         ids=["q5x50-p2x60", "q4x50-p3x50", "q3x60-p8x60", "q2-p1x60"])
@pytest.mark.parametrize("flags", [0, T])
def test_t_1_is_the_approximate_mod_down_word_for_word(oracle, qbits, pbits, flags):
    primes, roots = rs.chain(oracle, N, qbits + pbits)
    limbs = km._operand(oracle, primes, roots, N, 2, flags, 5)
    got, t = bm.mod_down_bgv(oracle, primes, roots, len(pbits), limbs, N, 1, flags)
    want, tw = km.mod_down(oracle, primes, roots, len(pbits), limbs, N, flags)
    for a, b in zip(got + t, want + tw):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("np_", [1, 2, 16])
def test_edge_words_against_python_integers(oracle, np_):
    """t_j in {0, 1, (p - 1) / 2, (p + 1) / 2, p - 1} x c in {0, q - 1} x T in {1, 2, 65537, 60 bits above every kept prime, q_0}: the
    model's words are the definition's, formed literally with Python integers"""
    primes, roots = rs.chain(oracle, N, [50, 52, 60] + [60] * np_)
    nq, pr = 3, primes[3:]
    coef = bm.plant([oracle.fill_uniform(N, q, 40 + l) for l, q in enumerate(primes)], primes, nq, N, 1)
    for pt in bm.edge_ts(primes):
        got, _ = bm.mod_down_bgv(oracle, primes, roots, np_, coef, N, pt, 0)
        for l, q in enumerate(primes[:nq]):
            want = [bm.word_int(pr, [coef[nq + j][i] for j in range(np_)], q, coef[l][i], pt) for i in range(N)]
            assert got[l].tolist() == want, (pt, l)


def test_toy_bgv_multiplication_decrypts(oracle):
    """N = 64, Q = 4 x 50 bits, P = 2 x 60 bits, two digits of two limbs, T = 65537, real encryptions under a ternary key, ModUp overshoot,
    keys with noise T e: after the key-switch ModDown the product decrypts to m1 m2 (no factor: P s^2 divides exactly), after the switch
    by q_L to m1 m2 q_L^-1 mod T"""
    nq, npp = 4, 2
    primes, roots = rs.chain(oracle, N, [50] * nq + [60] * npp)
    rng = random.Random(2025)
    bgv = bm.Bgv(oracle, primes, roots, nq, 2, N, PT, rng)
    m1, m2 = ([rng.randrange(PT) for _ in range(N)] for _ in range(2))
    ct1, ct2 = bgv.encrypt(m1), bgv.encrypt(m2)
    assert bgv.decrypt(ct1, nq) == m1 and bgv.decrypt(ct2, nq) == m2
    switched, relin, (d0, d1, d2, _) = bgv.multiply(ct1, ct2, bgv.relin_keys())
    want = bgv.plain_product(m1, m2)
    assert bgv.decrypt((d0, d1, d2), nq) == want, "the tensor alone"
    assert bgv.decrypt(relin, nq) == want, "after relinearisation"
    f = pow(primes[nq - 1], -1, PT)
    assert bgv.decrypt(switched, nq - 1) == [v * f % PT for v in want], "after the modulus switch"
    assert f != 1


# ---------------------------------------------------------------- the host side of csrc/ntt_bgv.h

@pytest.fixture(scope="module")
def host_check():
    return children.build_host_check("bgv_host_check")


@pytest.mark.parametrize("qbits,np_", [([30, 50, 52, 60], 1), ([50, 50, 60], 2), ([50] * 5, 4), ([52] * 16, 16)],
                         ids=["np1", "np2", "np4", "np16"])
def test_host_functions_equal_int128_and_the_model(oracle, host_check, tmp_path, qbits, np_):
    """bgv_sub_plain, bgv_sub_folded, bgv_digit1 and bgv_word of csrc/ntt_bgv.h, compiled for the host with the sanitizers, on the edge
    words and on random words: the program compares them with each other and with 128-bit integers, this test its output with the model"""
    primes, roots = rs.chain(oracle, N, qbits + [60] * np_)
    nq = len(qbits)
    coef = bm.plant([oracle.fill_uniform(N, q, 60 + l) for l, q in enumerate(primes)], primes, nq, N, 1)
    for pt in bm.edge_ts(primes):
        path = os.path.join(str(tmp_path), "vec.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d\n%s\n%s\n" % (np_, nq, pt, N, " ".join(map(str, primes[nq:])), " ".join(map(str, primes[:nq]))))
            for i in range(N):
                f.write(" ".join(str(int(coef[l][i])) for l in list(range(nq, nq + np_)) + list(range(nq))) + "\n")
        r = subprocess.run([host_check, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        got = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
        want, _ = bm.mod_down_bgv(oracle, primes, roots, np_, coef, N, pt, 0)
        for l in range(nq):
            assert [row[l] for row in got] == want[l].tolist(), (pt, l)


# ---------------------------------------------------------------- build checks

SIGNATURES = {
    "ntt_rns_mod_down_bgv_batch": "int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t batch, unsigned flags, void *stream",
    "ntt_rns_mod_down_bgv_batch_strided": "int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t limb_stride, "
                                          "uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream",
    "ntt_rns_mod_down_bgv_add_batch": "int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t, uint64_t batch, "
                                      "unsigned flags, void *stream",
    "ntt_rns_mod_down_bgv_add_batch_strided": "int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t, "
                                              "uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t a_limb_stride, uint64_t a_poly_stride, "
                                              "uint64_t batch, unsigned flags, void *stream",
}


def test_exports_the_four_symbols_with_the_documented_signatures(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SIGNATURES) <= names
    assert set(SIGNATURES) <= set(lib.EXPORTED_SYMBOLS)
    assert callable(lib.rns_mod_down_bgv) and callable(lib.rns_mod_down_bgv_add)
    with open(os.path.join(ROOT, "include", "ntt_mi355x.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for name, args in SIGNATURES.items():
        assert "NTT_API int %s(%s);" % (name, args) in header, name
    assert re.search(r"NTT_OPT_BGV_FUSED\s*=\s*21\b", header)
    assert lib.OPT_BGV_FUSED == 21


def test_bgv_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_bgv_mul", *children.STRICT))


def test_bgv_objects_hold_exactly_the_expected_instances_without_spills():
    """ksbgv_f64*.o: one moddown_bgv_fwd_kernel per (policy, class, LOGN) of the launch cases, none spilling vector registers or using
    scratch (where the objects are not at hand: the same kernels of the linked library)"""
    import glob

    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "ksbgv_*.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if "moddown_bgv_" in k["name"]]
    names = [k["name"] for k in ks]
    by = {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}
    want = rs.kernel_names("moddown_bgv_fwd_kernel", rs.fused_launch_cases())
    assert len(want) == 36
    assert set(by) == want, ("missing %s, unexpected %s" % (sorted(want - set(by))[:8], sorted(set(by) - want)[:8]))
    bad = {n: (k.get("vgpr_spill_count"), k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size")) for n, k in by.items()
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0) or k.get("group_segment_fixed_size", 0) > 160 * 1024}
    assert not bad, "spills / scratch / LDS: %s" % bad
