"""GPU: ntt_rns_mod_up_mul_batch and its strided form, c^ (+)= fwd(ModUp(digit)) (.) key^.  Every word of c^ against the model of
tests/modup_mul_model.py: every modup_mul_kernel instance (FP64 digits, a 60-bit digit feeding an FP64 run), the route proof without
a profiler (the sentinel in d_ext's other slots survives the fused route and is overwritten with ModUp's words by the composition, c^
bit for bit equal), the loop shapes, digit positions, layouts with canaries, lazy key words, the composition route (integer
policies, N = 2^15, N = 2^5, mixed chains), argument errors that write nothing, the plain-C example against examples/rns_key_switch.c
and the model, and one kernel trace: all 36 instances launched, the route call's launches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import children
import kernel_inventory
import keyswitch_model as km
import modup_mul_model as mm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "modup_mul_model.py")
L, B, A = mm.LAZY_IN, mm.BROADCAST, mm.ACCUMULATE


def _destroy(plans):
    for p in plans:
        p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_instance(lib, oracle, pol, k, logn):
    """each modup_mul_kernel<policy, LOGN, class>: three limbs of the class and two 60-bit limbs; digits of one and of two FP64
    limbs, and the 60-bit digit feeding the FP64 run (its own run on the composition); accumulate and broadcast each way"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    primes, roots = rs.chain(lib, n, [b, b, b, 60, 60])
    plans = rs.plans(lib, n, primes, roots)
    try:
        for (first, count), flags in (((0, 1), 0), ((1, 2), A | B), ((3, 2), B)):
            _, ext, _ = mm.run(lib, oracle, primes, roots, first, count, n, 3 if logn < 9 else 2, flags, fused=1, seed=logn + first, plans=plans)
            fp64 = [l for l in range(3) if not first <= l < first + count]
            assert [l for l in mm.untouched(ext, first, count) if l < 3] == fp64, "the FP64 run did not take the fused kernel"
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nlimbs,first,count", [(14, 17, 0, 1), (9, 6, 2, 3), (12, 20, 15, 3), (13, 18, 2, 16)])
def test_route_proof_by_the_sentinel(lib, oracle, logn, nlimbs, first, count):
    """an all-FP64 chain.  NTT_OPT_MODUP_FUSED 1: the sentinel in every non-digit slot of d_ext survives, the digit is unchanged;
    0: the same c^ bit for bit, the slots hold ntt_rns_mod_up_batch's words"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    plans = rs.plans(lib, n, primes, roots)
    digit = range(first, first + count)
    try:
        c1, ext1, up = mm.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=1, seed=3, plans=plans)
        assert mm.untouched(ext1, first, count) == [l for l in range(nlimbs) if l not in digit], "a slot of d_ext was written"
        for l in digit:
            assert np.array_equal(ext1[l], up[l]), "digit limb %d changed" % l
        c0, ext0, _ = mm.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=0, seed=3, plans=plans)
        for l in range(nlimbs):
            assert np.array_equal(c0[l], c1[l]), "c^ limb %d: the routes differ" % l
            assert np.array_equal(ext0[l], up[l]), "d_ext limb %d is not ModUp's" % l
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,first,count", [([50, 60, 60], 1, 2), ([50, 50], 0, 1)], ids=["two-workgroups", "one-workgroup-per-limb"])
def test_grid_stride_loop_wraps(lib, oracle, bits, first, count):
    """2^14, 5 polynomials, NTT_OPT_MAX_GRID 2: two workgroups for the one FP64 limb (rounds of 2, 2 and 1 blocks), or one per limb"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, bits)
    mm.run(lib, oracle, primes, roots, first, count, n, 5, A | B, fused=1, seed=14, max_grid=2)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,batch", [(8, 73), (8, 1), (10, 130), (6, 5)])
def test_batches(lib, oracle, logn, batch):
    """several blocks per workgroup with the last group partly dead (2^8: 73), one polynomial, 130"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60])
    mm.run(lib, oracle, primes, roots, 1, 2, n, batch, A, fused=1, seed=batch)
    mm.run(lib, oracle, primes, roots, 3, 1, n, batch, B, fused=1, seed=batch + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs,first,count", [(6, 0, 2), (6, 2, 2), (6, 4, 2), (5, 2, 1), (20, 2, 16), (17, 0, 1), (17, 16, 1), (34, 16, 3),
                                                (34, 18, 16), (34, 0, 16)])
@pytest.mark.parametrize("fused", [1, -1])
def test_digit_positions(lib, oracle, nlimbs, first, count, fused):
    """digits at the start, in the middle and at the end (inside P), of 1 and of 16 limbs, chains of more than 16 limbs"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 3) + [60, 60])
    mm.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=fused, seed=nlimbs + first)


@pytest.mark.gpu
def test_digit_of_largest_words(lib, oracle):
    """every digit word b_i - 1 over 16 limbs: the largest 128-bit sum"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * 18)
    mm.run(lib, oracle, primes, roots, 1, 16, n, 2, A, fused=1, seed=5, digit_max=True)
    primes, roots = rs.chain(lib, n, [60] * 16 + [50, 52])
    mm.run(lib, oracle, primes, roots, 0, 16, n, 2, B, fused=1, seed=6, digit_max=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [A, B, A | B])
def test_layouts(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    mm.run(lib, oracle, primes, roots, 1, 2, n, 3, flags, layout=layout, fused=1, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("flags", [L, L | A | B])
def test_lazy_key_words(lib, oracle, flags, fused):
    """key words up to min(4q, 2^53) - 1"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 51, 30, 52, 50])
    mm.run(lib, oracle, primes, roots, 0, 1, n, 3, flags, fused=fused, seed=21)


@pytest.mark.gpu
@pytest.mark.parametrize("arith,bits", [("auto", 60), ("u64", 60), ("r4", 60), ("u64", 58), ("r4", 58)])
def test_composition_integer_policies(lib, oracle, arith, bits):
    """NTT_ARITH_AUTO / U64 / U64_R4 plans for a run of 60-bit primes (the wide integer policy, or the radix-4 formulation, which
    admits q < 2^60), and 58-bit primes under the two explicit policies as the rescale, key-switch and Galois tests take them: every
    run on the composition, whatever NTT_OPT_MODUP_FUSED says"""
    n = 1 << 12
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [bits] * 5)
    plans = rs.plans(lib, n, primes, roots, a)
    try:
        _, ext, up = mm.run(lib, oracle, primes, roots, 1, 2, n, 3, A | B, fused=1, seed=7, plans=plans)
        assert not mm.untouched(ext, 1, 2), "an integer-policy run cannot take the fused kernel"
        mm.run(lib, oracle, primes, roots, 4, 1, n, 3, 0, fused=1, seed=8, plans=plans)
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [5, 15])
def test_composition_outside_the_fused_sizes(lib, oracle, logn):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60, 60])
    _, ext, _ = mm.run(lib, oracle, primes, roots, 1, 2, n, 2, A | B, fused=1, seed=logn)
    assert not mm.untouched(ext, 1, 2)
    mm.run(lib, oracle, primes, roots, 3, 2, n, 2, 0, fused=1, seed=logn + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0, -1])
@pytest.mark.parametrize("first,count", [(0, 2), (2, 3), (6, 2)])
def test_mixed_chains(lib, oracle, first, count, fused):
    n = 1 << 12
    primes, roots = rs.chain(lib, n, [60, 50, 50, 52, 50, 30] + [60, 60])
    mm.run(lib, oracle, primes, roots, first, count, n, 3, A | B, fused=fused, seed=first)


def _inverse_only_plan(lib, n, q, w):
    """a plan built from the inverse table alone: ntt_plan_create_from_tables with w_powers = NULL"""
    logn = n.bit_length() - 1
    winv = pow(w, -1, q)
    rev = [int(format(i, "0%db" % logn)[::-1], 2) if logn else 0 for i in range(n)]
    powers = np.array([pow(winv, r, q) for r in rev], dtype=np.uint64)
    h = C.c_void_p()
    rc = lib._lib.ntt_plan_create_from_tables(C.byref(h), 0, n, q, None, powers.ctypes.data_as(lib.U64P), lib.ARITH_AUTO)
    assert rc == 0, lib._lib.ntt_last_error()
    p = object.__new__(lib.Plan)
    p.h, p.N, p.q, p.root, p.device = h.value, n, q, w, 0
    return p


@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50] * 18)
    plans = rs.plans(lib, n, primes, roots)
    q2 = lib.find_prime(50, 2 * n)
    other = lib.Plan(2 * n, q2, lib.min_root(q2, 2 * n))
    same = lib.Plan(n, primes[0], roots[0])
    inv_only = _inverse_only_plan(lib, n, primes[3], roots[3])
    words = 18 * batch * n
    imgs = [oracle.fill_uniform(words, primes[0], 5 + i) for i in range(3)]
    dc, dext, dk = [lib.DeviceBuffer(words).upload(i) for i in imgs]
    p4 = plans[:4]
    four = 4 * batch * n
    bad = [
        ("count 0", p4, 0, 0, 0, None, {}),
        ("count 17", plans, 0, 17, 0, None, {}),
        ("digit past the end", p4, 3, 2, 0, None, {}),
        ("negative first", p4, -1, 2, 0, None, {}),
        ("differing N", [plans[0], other, plans[2], plans[3]], 0, 1, 0, None, {}),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 0, 1, 0, None, {}),
        ("unknown flag", p4, 0, 1, 8, None, {}),
        ("overlapping strides", p4, 0, 1, 0, (n, n), {}),
        ("null c", p4, 0, 1, 0, None, {"c": None}),
        ("null ext", p4, 0, 1, 0, None, {"ext": None}),
        ("null key", p4, 0, 1, 0, None, {"key": None}),
        ("a plan without its forward table", [plans[0], plans[1], plans[2], inv_only], 0, 1, 0, None, {}),
        ("c^ is d_ext", p4, 0, 1, A, None, {"c": dext.ptr}),
        ("c^ starts inside d_ext", p4, 0, 1, 0, None, {"c": dext.ptr + 8 * (four - 1)}),
        ("d_ext starts inside c^", p4, 0, 1, 0, None, {"ext": dc.ptr + 8 * (four - 1)}),
    ]
    try:
        for fused in (1, 0):
            plans[0].set_option(lib.OPT_MODUP_FUSED, fused)
            for what, ps, first, count, flags, lay, ptr in bad:
                with pytest.raises(lib.NttError):
                    lib.rns_mod_up_mul(ps, ptr.get("c", dc.ptr), ptr.get("ext", dext.ptr), first, count, ptr.get("key", dk.ptr), batch, flags,
                                       layout=lay)
                for buf, img in zip((dc, dext, dk), imgs):
                    assert np.array_equal(buf.download(), img), what
        # c^ right behind d_ext's last word is no overlap; c^ may alias the key (ntt_rns_fwd_mul_batch's rule)
        lib.rns_mod_up_mul(p4, dext.ptr + 8 * four, dext.ptr, 0, 1, dk.ptr, batch, 0)
        lib.rns_mod_up_mul(p4, dk.ptr, dext.ptr, 0, 1, dk.ptr, batch, 0)
    finally:
        dc.free(), dext.free(), dk.free()
        _destroy(plans + [other, same, inv_only])


def _checksums(lib, name):
    return [line for line in children.run_example(lib, name).splitlines() if line.startswith("poly ")]


@pytest.mark.gpu
def test_fused_example_prints_the_lines_of_the_two_call_example(lib, oracle):
    fused = _checksums(lib, "rns_key_switch_fused")
    assert len(fused) == 16
    assert fused == _checksums(lib, "rns_key_switch")  # (started only after the first exited 0)
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in (re.match(r"poly (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", line) for line in fused)}
    n, nq, np_, alpha = 1 << 13, 8, 2, 2
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(7)] + [lib.find_prime(60, n, k) for k in (1, 2)]
    roots = [lib.min_root(q, n) for q in primes]
    for p in range(2):
        acc = [np.zeros(n, dtype=np.uint64) for _ in primes]
        for k in range(4):
            digit = [oracle.fill_uniform(n, primes[l], 100 + 16 * p + l) for l in range(alpha * k, alpha * (k + 1))]
            key = [oracle.fill_uniform(n, q, 1000 + 16 * k + l) for l, q in enumerate(primes)]
            acc, _ = mm.model(oracle, primes, roots, digit, key, acc, n, 1, alpha * k, alpha, A | B)
        out, _ = km.mod_down(oracle, primes, roots, np_, acc, n, km.TRANSFORMED)
        for l in range(nq):
            assert got[(p, l)] == oracle.checksum(out[l]), (p, l)


@pytest.mark.gpu
def test_launch_proof_every_instance_and_the_route_call():
    """one traced child (tests/modup_mul_model.py): all 36 instances launched; the route call (2^14, 16 x 50-bit + 2 x 60-bit, digit
    (0, 2), NTT_OPT_MODUP_FUSED 1) is the only launch of modup_mul_kernel<ArithF64,14,1>, no FP64 fwd_mul_kernel runs anywhere in
    the child and bconv_kernel only once, for the route call's two 60-bit limbs (the child itself checks that the FP64 run's slots of
    d_ext keep the sentinel)"""
    launched = children.traced(MODEL_PY, [], 600)
    want = rs.kernel_names("modup_mul_kernel", rs.fused_launch_cases())
    assert len(want) == 36
    assert not sorted(want - set(launched)), "instances never launched: %s" % sorted(want - set(launched))
    assert launched.count("modup_mul_kernel<ArithF64,14,1>") == 1, launched
    # the forward-multiply launches of the child, parsed: the route call's 60-bit run has one (so the list is not empty), and none is
    # of an FP64 policy -- no FP64 run of any call went through the composition
    muls = [i for i in map(kernel_inventory.parse, launched) if i.family == "fwd_mul_kernel"]
    assert muls, launched
    assert all(i.policy.startswith("ArithU64") for i in muls), [i.key for i in muls]
    assert launched.count("bconv_kernel") == 1, launched
