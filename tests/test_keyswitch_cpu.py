"""CPU: ModUp / ModDown (ntt_rns_mod_up_batch, ntt_rns_mod_down_batch) without a GPU -- the model of tests/keyswitch_model.py against
the definitions over the CRT (ModUp: x + u B with 0 <= u < count; ModDown: round / floor(x / P) - v with 0 <= v < np) on edge and
random values, ModDown with one P prime against the rescale model word for word, the exported symbols, the plain-C example against
the public header alone, and the kernels of the new translation units (keyswitch_*.o): exactly the expected instances, none
spilling vector registers or using scratch."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import children
import keyswitch_model as km
import rescale_model as rm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")
LIB = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
T, F = km.TRANSFORMED, km.FLOOR
N = 64


# (Q bits, P bits): the chains the issue checked with Python integers
DOWN_CHAINS = [([50] * 16, [60]), ([50] * 16, [60, 60]), ([50] * 16, [50, 50, 50]), ([50] * 12, [60] * 4), ([60] * 20, [60] * 8),
               ([30] * 4, [52] * 16)]
DOWN_IDS = ["q16x50-p1x60", "q16x50-p2x60", "q16x50-p3x50", "q12x50-p4x60", "q20x60-p8x60", "q4x30-p16x52"]


def _down_values(Q, P, count, rng):
    """x = 0, QP - 1, the rounding boundaries k P + h, k P + h + 1, k P - 1, and random values"""
    M, h = Q * P, (P - 1) // 2
    xs = [0, M - 1, h, h + 1, P - 1, P]
    while len(xs) < count:
        k = rng.randrange(1, Q)
        xs += [k * P + h, k * P + h + 1, k * P - 1, rng.randrange(M)]
    return xs[:count]


@pytest.mark.parametrize("qbits,pbits", DOWN_CHAINS, ids=DOWN_IDS)
@pytest.mark.parametrize("flags", [0, F, T, T | F])
def test_mod_down_model_equals_the_definition(oracle, qbits, pbits, flags):
    primes, roots = rs.chain(oracle, N, qbits + pbits)
    np_, nq = len(pbits), len(qbits)
    Q, P = km.prod(primes[:nq]), km.prod(primes[nq:])
    rng = random.Random(hash((tuple(qbits), tuple(pbits), flags)) & 0xFFFF)
    xs = _down_values(Q, P, N, rng)
    coef = km.residues(xs, primes)
    limbs = [oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    got, t = km.mod_down(oracle, primes, roots, np_, limbs, N, flags)
    for j in range(np_):
        assert np.array_equal(t[j], coef[nq + j]), "t is the P limbs' coefficients"
    got = [oracle.ctx(N, q, w).inv(g) for q, w, g in zip(primes, roots, got)] if flags & T else got
    h = 0 if flags & F else (P - 1) // 2
    sums = km.fastbconv_int(primes[nq:], [c for c in coef[nq:]], None if flags & F else [h % p for p in primes[nq:]])
    for i, x in enumerate(xs):
        r = (x + h) % P
        assert (sums[i] - r) % P == 0
        v = (sums[i] - r) // P
        assert 0 <= v < np_, "v = %d outside [0, %d) for x = %d" % (v, np_, x)
        y = (x + h) // P - v
        for l, q in enumerate(primes[:nq]):
            assert int(got[l][i]) == y % q, "limb %d, x = %d" % (l, x)


@pytest.mark.parametrize("bits,first,count", km.UP_CHAINS, ids=["start", "middle", "end", "one-limb", "count16"])
@pytest.mark.parametrize("flags", [0, T])
def test_mod_up_model_equals_the_definition(oracle, bits, first, count, flags):
    primes, roots = rs.chain(oracle, N, bits)
    basis = primes[first:first + count]
    B = km.prod(basis)
    rng = random.Random(len(bits) * 31 + first + flags)
    xs = [0, B - 1, 1, B // 2] + [rng.randrange(B) for _ in range(N - 4)]
    coef = [oracle.fill_uniform(N, q, 50 + l) for l, q in enumerate(primes)]
    for i, q in enumerate(basis):
        coef[first + i] = np.array([x % q for x in xs], dtype=np.uint64)
    limbs = [oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    got = km.mod_up(oracle, primes, roots, limbs, N, first, count, flags)
    sums = km.fastbconv_int(basis, coef[first:first + count])
    for i, x in enumerate(xs):
        assert (sums[i] - x) % B == 0
        u = (sums[i] - x) // B
        assert 0 <= u < count, "u = %d outside [0, %d)" % (u, count)
    for l, (q, w) in enumerate(zip(primes, roots)):
        if first <= l < first + count:
            assert np.array_equal(got[l], limbs[l]), "the digit's limb %d changed" % l
            continue
        c = oracle.ctx(N, q, w).inv(got[l]) if flags & T else got[l]
        assert c.tolist() == [s % q for s in sums], "limb %d" % l


@pytest.mark.parametrize("bits", [[50, 50, 50, 52], [50, 50, 30], [50, 30, 60], [60, 50, 50, 50], [30, 50]])
@pytest.mark.parametrize("flags", [0, F, T, T | F])
def test_mod_down_with_one_p_prime_is_the_rescale(oracle, bits, flags):
    primes, roots = rs.chain(oracle, N, bits)
    coef = [oracle.fill_uniform(2 * N, q, 70 + l) for l, q in enumerate(primes)]
    limbs = [oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    got, t = km.mod_down(oracle, primes, roots, 1, limbs, N, flags)
    want, tr = rm.model(oracle, primes, roots, limbs, N, flags)
    for l in range(len(primes) - 1):
        assert np.array_equal(got[l], want[l]), "limb %d" % l
    assert np.array_equal(t[0], tr)


def test_exports_the_four_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"ntt_rns_mod_up_batch", "ntt_rns_mod_up_batch_strided", "ntt_rns_mod_down_batch", "ntt_rns_mod_down_batch_strided"} <= names


def test_key_switch_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_key_switch", *children.STRICT))


def expected_instances():
    fwd = rs.kernel_names("moddown_fwd_kernel", rs.fused_launch_cases())
    return fwd | {"moddown_coef_kernel", "bconv_kernel"}


def keyswitch_kernels():
    """{normalised name: metadata} of every kernel in the keyswitch translation units (or, where the objects are not at hand, the
    key-switching kernels of the linked library)"""
    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "keyswitch_*.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if "moddown" in k["name"] or "bconv_kernel" in k["name"]]
    names = [k["name"] for k in ks]
    return {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}


def test_keyswitch_objects_hold_exactly_the_expected_instances_without_spills():
    ks = keyswitch_kernels()
    want = expected_instances()
    assert len(want) == 38
    assert set(ks) == want, ("missing %s, unexpected %s" % (sorted(want - set(ks))[:8], sorted(set(ks) - want)[:8]))
    assert not any("rescale" in n or "fused_kernel" in n for n in ks)
    bad = {n: (k.get("vgpr_spill_count"), k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size"))
           for n, k in ks.items()
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0) or k.get("group_segment_fixed_size", 0) > 160 * 1024}
    assert not bad, "spills / scratch / LDS: %s" % bad
