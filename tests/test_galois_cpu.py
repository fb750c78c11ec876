"""CPU: the Galois automorphisms and the rotation key product (ntt_galois_batch, ntt_rns_galois_batch, ntt_rns_galois_dot_batch)
without a GPU -- the model of tests/galois_model.py against the oracle's transforms and schoolbook products (both domains agree,
sigma_g sigma_h = sigma_gh, sigma_g is multiplicative, the key product), the tile property of the NTT-domain permutation, the
kernels' index functions and 128-bit reduction compiled for the host (tools/galois_index_probe.hip) against the model and Python
integers, the exported symbols, the plain-C example against the public header alone, and the kernels of the new translation unit
(galois_*.o): exactly the expected names, none spilling vector registers or using scratch."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import children
import galois_model as gm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")
LIB = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
BITS = [30, 50, 52, 60]


def _edges(orc, n, q, seed, batch=1):
    a = orc.fill_uniform(batch * n, q, seed)
    rs.edge_fill(a, q)
    return a


@pytest.mark.parametrize("n", [64, 256])
def test_both_domains_agree_through_the_oracle(oracle, n):
    """fwd(coef_model(a, g)) == ntt_model(fwd(a), g)"""
    primes, roots = rs.chain(oracle, n, BITS)
    for q, w in zip(primes, roots):
        cx = oracle.ctx(n, q, w)
        a = _edges(oracle, n, q, 3, batch=2)
        for g in gm.g_list(n):
            assert np.array_equal(cx.fwd(gm.coef_model(a, n, g, q)), gm.ntt_model(cx.fwd(a), n, g)), (q, g)


@pytest.mark.parametrize("n", [64, 256])
def test_composition(oracle, n):
    """sigma_g o sigma_h = sigma_{gh mod 2N}, in both domains"""
    q = oracle.find_prime(50, n, 0)
    a = _edges(oracle, n, q, 5)
    gs = gm.g_list(n)
    for g in gs:
        for h in gs:
            gh = g * h % (2 * n)
            assert np.array_equal(gm.coef_model(gm.coef_model(a, n, h, q), n, g, q), gm.coef_model(a, n, gh, q)), (g, h)
            assert np.array_equal(gm.ntt_model(gm.ntt_model(a, n, h), n, g), gm.ntt_model(a, n, gh)), (g, h)


def test_multiplicative_against_the_schoolbook_product(oracle):
    """sigma_g(a) sigma_g(b) = sigma_g(a b) at N = 64"""
    n = 64
    primes, _ = rs.chain(oracle, n, BITS)
    for q in primes:
        a, b = _edges(oracle, n, q, 7), _edges(oracle, n, q, 8)
        ab = oracle.schoolbook(a, b, n, q)
        for g in gm.g_list(n):
            assert np.array_equal(oracle.schoolbook(gm.coef_model(a, n, g, q), gm.coef_model(b, n, g, q), n, q), gm.coef_model(ab, n, g, q)), (q, g)


@pytest.mark.parametrize("flags", [0, gm.ACCUMULATE, gm.KEY_BROADCAST, gm.ACCUMULATE | gm.KEY_BROADCAST])
def test_dot_model_is_the_sum_of_schoolbook_products(oracle, flags):
    """inv(dot_model) = (c +) sum_i sigma_g(a_i) key_i at N = 64, k = 3, two polynomials"""
    n, k, batch = 64, 3, 2
    primes, roots = rs.chain(oracle, n, BITS)
    for q, w in zip(primes, roots):
        cx = oracle.ctx(n, q, w)
        a = [_edges(oracle, n, q, 20 + i, batch) for i in range(k)]
        key = [oracle.fill_uniform(n if flags & gm.KEY_BROADCAST else batch * n, q, 30 + i) for i in range(k)]
        c = oracle.fill_uniform(batch * n, q, 40)
        for g in gm.g_list(n):
            got = cx.inv(gm.dot_model(oracle, cx.fwd(c), [cx.fwd(x) for x in a], [cx.fwd(x) for x in key], n, g, q, flags))
            for p in range(batch):
                want = c[p * n:(p + 1) * n].copy() if flags & gm.ACCUMULATE else np.zeros(n, dtype=np.uint64)
                for x, y in zip(a, key):
                    yp = y if flags & gm.KEY_BROADCAST else y[p * n:(p + 1) * n]
                    want = (want + oracle.schoolbook(gm.coef_model(x[p * n:(p + 1) * n], n, g, q), yp, n, q)) % np.uint64(q)
                assert np.array_equal(got[p * n:(p + 1) * n], want), (q, g, p)


def test_tile_property():
    """for every tile size 2^b the outputs of one aligned storage tile come from exactly one aligned storage tile of the input"""
    n, m = 1 << 10, 10
    for g in [3, 5, 25, pow(5, 1000, 2 * n), 2 * n - 1]:
        src = gm.ntt_source(n, g)
        assert sorted(src.tolist()) == list(range(n)), "a permutation"
        for b in range(m + 1):
            tiles = (src >> b).reshape(-1, 1 << b)
            assert (tiles == tiles[:, :1]).all(), (g, b)


def test_rotation_helper(lib):
    for n in [2, 4, 64, 1 << 14]:
        for steps in [0, 1, 2, 7, n // 2 - 1, n // 2, 12345, -1, -3, -n]:
            assert lib.galois_rotation(n, steps) == gm.rotation(n, steps), (n, steps)
    for bad in [0, 1, 3, 48]:
        assert lib.galois_rotation(bad, 1) == 0


@pytest.fixture(scope="module")
def probe():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "galois_index_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "internal"), "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tools", "galois_index_probe.hip")])
    return exe


def test_index_functions_equal_the_model(probe):
    """galois_ntt_src / galois_coef_src of csrc/ntt_galois.h, compiled for the host, on every slot"""
    cases = [(n, g) for n in [2, 4, 64, 1 << 14] for g in gm.g_list(n)]
    out = subprocess.check_output([probe] + [str(v) for c in cases for v in c], text=True)
    blocks = out.split("#")[1:]
    assert len(blocks) == len(cases)
    for (n, g), blk in zip(cases, blocks):
        lines = blk.splitlines()
        assert lines[0].split() == [str(n), str(g)]
        got = np.array([l.split() for l in lines[1:]], dtype=np.int64)
        assert got.shape == (n, 3)
        src, neg = gm.coef_source(n, g)
        assert np.array_equal(got[:, 0], gm.ntt_source(n, g)), (n, g)
        assert np.array_equal(got[:, 1], src) and np.array_equal(got[:, 2], neg.astype(np.int64)), (n, g)


@pytest.mark.parametrize("bits", [60, 30])
def test_sum_of_32_extreme_products_reduces_exactly(oracle, probe, bits):
    """bconv_mac / bconv_reduce with k = 32 operands all q - 1 and c = q - 1 against Python integers: 32 (2^61)^2 + 2^61 < 2^128"""
    n = 64
    q = max(oracle.find_prime(bits, n, k) for k in range(4)) if bits == 60 else oracle.find_prime(bits, n, 0)
    for k in (1, 32):
        hi, lo, v = (int(x) for x in subprocess.check_output([probe, "--reduce", str(q), str(k), str(q - 1)], text=True).split())
        s = k * (q - 1) * (q - 1) + (q - 1)
        assert s < 1 << 128 and (hi << 64) + lo == s
        assert v == s % q


NAMES = ["ntt_galois_rotation", "ntt_galois_batch", "ntt_rns_galois_batch", "ntt_rns_galois_batch_strided", "ntt_rns_galois_dot_batch",
         "ntt_rns_galois_dot_batch_strided"]


def test_exports_the_six_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    assert set(NAMES) <= set(lib.EXPORTED_SYMBOLS)
    assert (lib.GALOIS_TRANSFORMED, lib.GALOIS_ACCUMULATE, lib.GALOIS_KEY_BROADCAST) == (1, 2, 4)


def test_rotate_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_rotate", *children.STRICT))


EXPECTED = {"galois_ntt_kernel<true>", "galois_ntt_kernel<false>", "galois_coef_kernel", "galois_dot_kernel"}


def galois_kernels():
    """{normalised name: metadata} of every kernel in the galois translation units (or, where the objects are not at hand, the
    galois kernels of the linked library)"""
    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "galois_*.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else [k for k in check_spills.kernels_of(LIB) if "galois" in k["name"]]
    names = [k["name"] for k in ks]
    return {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}


def test_galois_objects_hold_exactly_the_expected_kernels_without_spills():
    ks = galois_kernels()
    assert set(ks) == EXPECTED, ("missing %s, unexpected %s" % (sorted(EXPECTED - set(ks)), sorted(set(ks) - EXPECTED)))
    bad = {n: (k.get("vgpr_spill_count"), k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size"))
           for n, k in ks.items()
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0) or k.get("group_segment_fixed_size", 0) > 160 * 1024}
    assert not bad, "spills / scratch / LDS: %s" % bad
