"""CPU: the ciphertext tensor product and ModDown into a ciphertext (ntt_rns_tensor_batch, ntt_rns_mod_down_add_batch) without a GPU --
the model of tests/ct_mul_model.py against the definitions (the tensor through the oracle's transforms and negacyclic products; the
accumulating ModDown over the CRT: c + round / floor(x / P) - v with 0 <= v < np; one P prime against the rescale model), the
exported symbols, the header as C and C++, the plain-C example against the public header alone, and the kernels of the new
translation units (ksfold_*.o, ct_elem.o): exactly the expected instances, none spilling vector registers or using scratch, none
carrying a name that an older test selects by substring."""
import glob
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import children
import ct_mul_model as cm
import keyswitch_model as km
import rescale_model as rm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")
LIB = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
T, F, A = cm.TRANSFORMED, cm.FLOOR, cm.ACCUMULATE
N = 64
SYMBOLS = {"ntt_rns_tensor_batch", "ntt_rns_tensor_batch_strided", "ntt_rns_mod_down_add_batch", "ntt_rns_mod_down_add_batch_strided"}
PINNED = ("moddown", "bconv_kernel", "rescale", "galois", "modup_mul", "fused_kernel", "keypair_dot2")


def _negacyclic(orc, n, q, w, x, y):
    """the oracle's negacyclic product of two coefficient vectors"""
    cx = orc.ctx(n, q, w)
    return cx.inv(orc.pointwise(cx.fwd(x), cx.fwd(y), q))


@pytest.mark.parametrize("bits", [[60, 50, 30, 52], [50] * 3], ids=["mixed", "50"])
def test_tensor_model_is_the_negacyclic_tensor(oracle, bits):
    """inv(c0), inv(c1), inv(c2) of the model on transformed operands are a0 b0, a0 b1 + a1 b0, a1 b1 in Z_q[X] / (X^N + 1)"""
    primes, roots = rs.chain(oracle, N, bits)
    coef = [[oracle.fill_uniform(2 * N, q, 10 * j + l) for l, q in enumerate(primes)] for j in range(4)]
    hat = [[oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, op)] for op in coef]
    c = cm.tensor(oracle, primes, *hat)
    for l, (q, w) in enumerate(zip(primes, roots)):
        a0, a1, b0, b1 = (coef[j][l] for j in range(4))
        inv = oracle.ctx(N, q, w).inv
        assert np.array_equal(inv(c[0][l]), _negacyclic(oracle, N, q, w, a0, b0))
        mid = (_negacyclic(oracle, N, q, w, a0, b1) + _negacyclic(oracle, N, q, w, a1, b0)) % np.uint64(q)
        assert np.array_equal(inv(c[1][l]), mid)
        assert np.array_equal(inv(c[2][l]), _negacyclic(oracle, N, q, w, a1, b1))


def test_tensor_model_takes_lazy_words(oracle):
    """words in [0, 4q) give what their residues give"""
    primes, _ = rs.chain(oracle, N, [60, 30])
    ops = cm.tensor_inputs(oracle, primes, N, 1, 5)
    lazy = [[v + np.uint64(3 * q) for v, q in zip(op, primes)] for op in ops]
    for x, y in zip(cm.tensor(oracle, primes, *ops), cm.tensor(oracle, primes, *lazy)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


DOWN_CHAINS = [([50] * 16, [60]), ([50] * 16, [60, 60]), ([50] * 12, [60] * 4), ([30] * 4, [52] * 16)]


@pytest.mark.parametrize("qbits,pbits", DOWN_CHAINS, ids=["q16x50-p1x60", "q16x50-p2x60", "q12x50-p4x60", "q4x30-p16x52"])
@pytest.mark.parametrize("flags", [A, A | F, A | T, A | T | F])
def test_accumulating_model_equals_the_definition(oracle, qbits, pbits, flags):
    """x in [0, QP) and c in [0, Q) held by the CRT: the model is c + round(x / P) - v mod Q with 0 <= v < np (FLOOR: floor)"""
    primes, roots = rs.chain(oracle, N, qbits + pbits)
    np_, nq = len(pbits), len(qbits)
    Q, P = km.prod(primes[:nq]), km.prod(primes[nq:])
    rng = random.Random(len(qbits) * 131 + len(pbits) * 7 + flags)
    h = 0 if flags & F else (P - 1) // 2
    xs = [0, Q * P - 1, h, h + 1, P - 1, P] + [rng.randrange(Q * P) for _ in range(N - 6)]
    cs = [0, Q - 1, Q - 1, 1] + [rng.randrange(Q) for _ in range(N - 4)]
    xc, cc = km.residues(xs, primes), km.residues(cs, primes[:nq])
    fwd = lambda limbs, pr, rt: [oracle.ctx(N, q, w).fwd(v) for q, w, v in zip(pr, rt, limbs)] if flags & T else limbs
    got, t = cm.mod_down_add(oracle, primes, roots, np_, fwd(cc, primes[:nq], roots[:nq]), fwd(xc, primes, roots), N, flags)
    for j in range(np_):
        assert np.array_equal(t[j], xc[nq + j]), "t is the P limbs' coefficients"
    got = [oracle.ctx(N, q, w).inv(g) for q, w, g in zip(primes, roots, got)] if flags & T else got
    assert km.crt(cc, primes[:nq]) == cs
    sums = km.fastbconv_int(primes[nq:], xc[nq:], None if flags & F else [h % p for p in primes[nq:]])
    for i, (x, c) in enumerate(zip(xs, cs)):
        r = (x + h) % P
        assert (sums[i] - r) % P == 0
        v = (sums[i] - r) // P
        assert 0 <= v < np_, "v = %d outside [0, %d)" % (v, np_)
        y = c + (x + h) // P - v
        for l, q in enumerate(primes[:nq]):
            assert int(got[l][i]) == y % q, "limb %d, x = %d, c = %d" % (l, x, c)


@pytest.mark.parametrize("bits", [[50, 50, 50, 52], [50, 30, 60], [60, 50, 50, 50]])
@pytest.mark.parametrize("flags", [0, A, A | F, T, A | T, A | T | F])
def test_one_p_prime_is_the_rescale_plus_the_addition(oracle, bits, flags):
    primes, roots = rs.chain(oracle, N, bits)
    nq = len(primes) - 1
    a = km._operand(oracle, primes, roots, N, 2, flags & T, 3)
    c = km._operand(oracle, primes[:nq], roots[:nq], N, 2, flags & T, 4)
    got, t = cm.mod_down_add(oracle, primes, roots, 1, c, a, N, flags)
    want, tr = rm.model(oracle, primes, roots, a, N, flags & (T | F))
    for l, q in enumerate(primes[:nq]):
        w = (c[l] + want[l]) % np.uint64(q) if flags & A else want[l]
        assert np.array_equal(got[l], w), "limb %d" % l
    assert np.array_equal(t[0], tr)


def test_exports_the_four_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOLS <= names, SYMBOLS - names
    assert SYMBOLS <= set(lib.EXPORTED_SYMBOLS)
    assert callable(lib.rns_tensor) and callable(lib.rns_mod_down_add)


def test_header_declares_the_flag_and_the_option(lib):
    header = open(os.path.join(ROOT, "include", "ntt_mi355x.h")).read()
    assert re.search(r"NTT_OPT_MODDOWN_ADD_FUSED\s*=\s*20\b", header)
    assert re.search(r"NTT_MODDOWN_ACCUMULATE\s*=\s*4\b", header)
    assert lib.OPT_MODDOWN_ADD_FUSED == 20 and lib.MODDOWN_ACCUMULATE == 4
    src = ('#include "ntt_mi355x.h"\nint main(void){return (NTT_MODDOWN_ACCUMULATE == 4 && NTT_OPT_MODDOWN_ADD_FUSED == 20 && '
           "ntt_rns_tensor_batch_strided && ntt_rns_mod_down_add_batch_strided && ntt_rns_tensor_batch && ntt_rns_mod_down_add_batch) ? 0 : 1;}\n")
    children.syntax_check(src)


def test_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_ciphertext_mul", *children.STRICT))


def expected_instances():
    fwd = rs.kernel_names("ksfold_fwd_kernel", rs.fused_launch_cases())
    return fwd | {"tensor_kernel", "ct_fold_kernel"}


def ct_mul_kernels():
    """{normalised name: metadata} of every kernel in the new translation units (or, where the objects are not at hand, the kernels
    of the linked library that carry their names)"""
    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "ksfold_*.o"))) + sorted(glob.glob(os.path.join(CSRC, "ct_elem.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if any(s in k["name"] for s in ("ksfold_fwd_kernel", "tensor_kernel", "ct_fold_kernel"))]
    names = [k["name"] for k in ks]
    return {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}


def test_new_objects_hold_exactly_the_expected_instances_without_spills():
    ks = ct_mul_kernels()
    want = expected_instances()
    assert len(want) == 38
    assert set(ks) == want, ("missing %s, unexpected %s" % (sorted(want - set(ks))[:8], sorted(set(ks) - want)[:8]))
    assert not any(s in n for n in ks for s in PINNED), "a kernel name carries a substring that an older test selects by"
    bad = {n: (k.get("vgpr_spill_count"), k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size"))
           for n, k in ks.items()
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0) or k.get("group_segment_fixed_size", 0) > 160 * 1024}
    assert not bad, "spills / scratch / LDS: %s" % bad


def test_host_object_instantiates_no_kernel_of_the_new_families():
    import check_spills
    host = os.path.join(CSRC, "ntt_host.o")
    names = [k["name"] for k in check_spills.kernels_of(host)] if os.path.exists(host) else []  # (a bare library: nothing to read)
    assert not any(s in n for n in names for s in ("ksfold", "tensor_kernel", "ct_fold_kernel")), names
