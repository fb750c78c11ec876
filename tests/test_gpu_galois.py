"""GPU: the Galois automorphisms and the rotation key product (ntt_galois_batch, ntt_rns_galois_batch, ntt_rns_galois_dot_batch and
their strided forms).  Every output word against the model of tests/galois_model.py, bit for bit: both domains over sizes 2 .. 2^16,
batches, limb counts across the 16-limb launch boundary, the issue's list of Galois elements, integer-policy plans, lazy and
all-ones words passing through the NTT-domain form, the key product with and without accumulation and a broadcast key up to k = 32
and all-(q - 1) operands, both domains and the dot tied together on the device, the four layouts with canaries, argument errors that
write nothing, the plain-C example; and one kernel trace: 17 limbs are two galois_ntt_kernel launches, a dot over 16 limbs is one
galois_dot_kernel."""
import os
import re

import numpy as np
import pytest

import children
import galois_model as gm
import rns_support as rs
import keyswitch_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "galois_model.py")
T, ACC, BC = gm.TRANSFORMED, gm.ACCUMULATE, gm.KEY_BROADCAST
MIXED = [60, 50, 52, 30]


def _bits(count):
    return (MIXED * ((count + 3) // 4))[:count]


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [1, 2, 6, 10, 14, 16])
@pytest.mark.parametrize("flags", [0, T], ids=["coef", "ntt"])
def test_sizes_and_galois_elements(lib, oracle, logn, flags):
    """every g of the list on a mixed chain, two polynomials (2^16: the first size where a polynomial exceeds any one workgroup's
    share)"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, MIXED if logn < 16 else [60, 30])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    limbs = gm.operand(oracle, primes, n, 2, logn)
    try:
        for g in gm.g_list(n):
            gm.run_galois(lib, oracle, primes, roots, n, 2, g, flags, plans=plans, limbs=limbs)
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 130])
@pytest.mark.parametrize("flags", [0, T], ids=["coef", "ntt"])
def test_batches(lib, oracle, batch, flags):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, MIXED)
    for g in (5, n + 1, 2 * n - 1):
        gm.run_galois(lib, oracle, primes, roots, n, batch, g, flags, seed=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [1, 5, 17, 34])
@pytest.mark.parametrize("flags", [0, T], ids=["coef", "ntt"])
def test_limb_counts_across_the_launch_boundary(lib, oracle, nlimbs, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, _bits(nlimbs))
    for g in (25, 2 * n - 1):
        gm.run_galois(lib, oracle, primes, roots, n, 2, g, flags, seed=nlimbs)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["auto", "u64", "r4"])
def test_integer_policy_plans_and_the_one_limb_form(lib, oracle, arith):
    """ARITH_U64 and ARITH_U64_R4 at 58 bits, AUTO at 60 bits; Plan.galois beside the RNS form"""
    n, batch = 1 << 12, 3
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58] * 3 if arith != "auto" else [60] * 3)
    plans = [lib.Plan(n, q, w, arith=a) for q, w in zip(primes, roots)]
    try:
        g = gm.rotation(n, 7)
        for flags in (0, T):
            gm.run_galois(lib, oracle, primes, roots, n, batch, g, flags, plans=plans, seed=4)
        gm.run_dot(lib, oracle, primes, roots, n, batch, 2, g, T, plans=plans, seed=5)
        x = gm.operand(oracle, primes[:1], n, batch, 6)[0]
        src, dst = lib.DeviceBuffer(x.size).upload(x), lib.DeviceBuffer(x.size)
        for flags in (0, T):
            plans[0].galois(dst.ptr, src.ptr, g, batch, flags)
            want = gm.ntt_model(x, n, g) if flags else gm.coef_model(x, n, g, primes[0])
            assert np.array_equal(dst.download(), want)
        src.free(), dst.free()
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
def test_ntt_domain_passes_lazy_words_through(lib, oracle):
    """words >= q (a lazy forward output, a buffer of 2^64 - 1) come out bit-identical"""
    n, batch = 1 << 12, 2
    primes, roots = rs.chain(lib, n, [50, 60])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    try:
        lazy = [p.fwd_host(oracle.fill_uniform(batch * n, q, 9), lazy=True) for p, q in zip(plans, primes)]
        ones = [np.full(batch * n, 2**64 - 1, dtype=np.uint64) for _ in primes]
        for limbs in (lazy, ones):
            for g in (3, 2 * n - 1):
                gm.run_galois(lib, oracle, primes, roots, n, batch, g, T, plans=plans, limbs=limbs)
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 16, 32])
@pytest.mark.parametrize("flags", [T, T | ACC, T | BC, T | ACC | BC], ids=["plain", "acc", "bcast", "acc-bcast"])
def test_dot(lib, oracle, k, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, _bits(5))
    gm.run_dot(lib, oracle, primes, roots, n, 2, k, gm.rotation(n, k), flags, seed=k)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [5, 18])
@pytest.mark.parametrize("logn", [6, 12, 14, 16])
def test_dot_sizes_and_limb_counts(lib, oracle, logn, nlimbs):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, _bits(nlimbs))
    gm.run_dot(lib, oracle, primes, roots, n, 2, 3, gm.rotation(n, -5), T | ACC | (BC if logn % 4 else 0), seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [T, T | ACC])
def test_dot_of_32_extreme_products(lib, oracle, flags):
    """every operand word q - 1, k = 32, 60-bit primes: the largest sum the 128-bit accumulator sees"""
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [60, 60, 60])
    gm.run_dot(lib, oracle, primes, roots, n, 2, 32, 2 * n - 1, flags, extreme=True)


@pytest.mark.gpu
def test_both_domains_and_the_dot_agree_on_the_device(lib, oracle):
    """rns_inv(dot) == sum_i sigma_g(a_i) key_i with the coefficient automorphism's outputs and rns_negacyclic_mul (N = 2^12, k = 3,
    4 limbs)"""
    n, batch, k = 1 << 12, 2, 3
    primes, roots = rs.chain(lib, n, MIXED)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    g = gm.rotation(n, 11)
    words = len(primes) * batch * n

    def dev(limbs):
        return lib.DeviceBuffer(words).upload(np.concatenate(limbs))

    a = [gm.operand(oracle, primes, n, batch, 50 + i) for i in range(k)]
    key = [gm.operand(oracle, primes, n, batch, 60 + i) for i in range(k)]
    bufs = []
    try:
        ahat, keyhat = [dev(x) for x in a], [dev(x) for x in key]
        dot = lib.DeviceBuffer(words)
        bufs += ahat + keyhat + [dot]
        for b in ahat + keyhat:
            lib.rns_fwd(plans, b.ptr, batch)
        lib.rns_galois_dot(plans, dot.ptr, [b.ptr for b in ahat], [b.ptr for b in keyhat], g, batch, T)
        lib.rns_inv(plans, dot.ptr, batch)
        got = dot.download()
        want = np.zeros(words, dtype=np.uint64)
        qs = np.repeat(np.array(primes, dtype=np.uint64), batch * n)
        for x, y in zip(a, key):
            src, rot, kb, prod = dev(x), lib.DeviceBuffer(words), dev(y), lib.DeviceBuffer(words)
            bufs += [src, rot, kb, prod]
            lib.rns_galois(plans, rot.ptr, src.ptr, g, batch, 0)
            lib.rns_negacyclic_mul(plans, prod.ptr, rot.ptr, kb.ptr, batch)
            want = (want + prod.download()) % qs
        assert np.array_equal(got, want)
    finally:
        for b in bufs:
            b.free()
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
def test_layouts(lib, oracle, layout):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, MIXED + [50])
    g = gm.rotation(n, 3)
    gm.run_galois(lib, oracle, primes, roots, n, 3, g, 0, layout=layout, seed=11)
    gm.run_galois(lib, oracle, primes, roots, n, 3, g, T, layout=layout, seed=12)
    gm.run_dot(lib, oracle, primes, roots, n, 3, 2, g, T | ACC, layout=layout, seed=13)
    gm.run_dot(lib, oracle, primes, roots, n, 3, 2, g, T | BC, layout=layout, seed=14)


@pytest.mark.gpu
def test_ntt_domain_with_operands_off_the_16_byte_grid(lib, oracle):
    """buffers that start 8 bytes off a 16-byte boundary (the one-slot-per-lane kernel) give the same words"""
    n, batch = 1 << 10, 3
    primes, roots = rs.chain(lib, n, [50, 60])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    limbs = gm.operand(oracle, primes, n, batch, 21)
    img = np.concatenate(limbs)
    src, dst = lib.DeviceBuffer(img.size + 2), lib.DeviceBuffer(img.size + 2)
    try:
        src.upload(np.concatenate([[rs.CANARY], img, [rs.CANARY]]).astype(np.uint64))
        dst.upload(np.full(img.size + 2, rs.CANARY, dtype=np.uint64))
        g = gm.rotation(n, 9)
        lib.rns_galois(plans, dst.ptr + 8, src.ptr + 8, g, batch, T)
        got = dst.download()
        assert got[0] == rs.CANARY and got[-1] == rs.CANARY
        assert np.array_equal(got[1:-1], np.concatenate([gm.ntt_model(x, n, g) for x in limbs]))
    finally:
        src.free(), dst.free()
        for p in plans:
            p.destroy()


@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch, nl = 1 << 10, 2, 3
    primes, roots = rs.chain(lib, n, [50] * nl)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    q2 = lib.find_prime(50, 2 * n)
    other = lib.Plan(2 * n, q2, lib.min_root(q2, 2 * n))
    words = nl * batch * n
    img_in, img_out = oracle.fill_uniform(words, primes[0], 5), oracle.fill_uniform(words, primes[0], 6)
    din, dout, dkey = lib.DeviceBuffer(words).upload(img_in), lib.DeviceBuffer(words).upload(img_out), lib.DeviceBuffer(words).upload(img_in)

    def untouched(what):
        assert np.array_equal(dout.download(), img_out) and np.array_equal(din.download(), img_in) and np.array_equal(dkey.download(), img_in), what

    L = lib._lib
    arr = lib._plan_array
    galois = [
        ("g even", plans, dout.ptr, din.ptr, 4, 0, None),
        ("g zero", plans, dout.ptr, din.ptr, 0, T, None),
        ("g = 2N", plans, dout.ptr, din.ptr, 2 * n, T, None),
        ("g > 2N", plans, dout.ptr, din.ptr, 2 * n + 1, 0, None),
        ("no limb", [], dout.ptr, din.ptr, 3, T, None),
        ("null output", plans, None, din.ptr, 3, T, None),
        ("null input", plans, dout.ptr, None, 3, T, None),
        ("differing N", [plans[0], other, plans[2]], dout.ptr, din.ptr, 3, T, None),
        ("unknown flag", plans, dout.ptr, din.ptr, 3, 8, None),
        ("ACCUMULATE passed to galois", plans, dout.ptr, din.ptr, 3, T | ACC, None),
        ("KEY_BROADCAST passed to galois", plans, dout.ptr, din.ptr, 3, T | BC, None),
        ("overlapping strides", plans, dout.ptr, din.ptr, 3, T, (n, n)),
        ("in place", plans, dout.ptr, dout.ptr, 3, T, None),
        ("output inside the input", plans, din.ptr + 8 * n, din.ptr, 3, 0, None),
    ]
    for what, ps, o, i, g, flags, lay in galois:
        with pytest.raises(lib.NttError):
            if lay:
                lib._check(L.ntt_rns_galois_batch_strided(len(ps), arr(ps), o, i, g, lay[0], lay[1], batch, flags, None))
            else:
                lib._check(L.ntt_rns_galois_batch(len(ps), arr(ps), o, i, g, batch, flags, None))
        untouched(what)
    with pytest.raises(lib.NttError):
        plans[0].galois(dout.ptr, din.ptr, 2, batch, T)
    with pytest.raises(lib.NttError):
        plans[0].galois(dout.ptr, dout.ptr + 8 * n, 3, batch, T)
    untouched("one-limb form")
    a2, k2 = [din.ptr, din.ptr], [dkey.ptr, dkey.ptr]
    dot = [
        ("g even", plans, dout.ptr, a2, k2, 2, T, None),
        ("g = 2N", plans, dout.ptr, a2, k2, 2 * n, T, None),
        ("no limb", [], dout.ptr, a2, k2, 3, T, None),
        ("k = 0", plans, dout.ptr, [], [], 3, T, None),
        ("k = 33", plans, dout.ptr, [din.ptr] * 33, [dkey.ptr] * 33, 3, T, None),
        ("null output", plans, None, a2, k2, 3, T, None),
        ("null operand", plans, dout.ptr, [din.ptr, None], k2, 3, T, None),
        ("null key", plans, dout.ptr, a2, [dkey.ptr, None], 3, T, None),
        ("differing N", [plans[0], other, plans[2]], dout.ptr, a2, k2, 3, T, None),
        ("unknown flag", plans, dout.ptr, a2, k2, 3, 8, None),
        ("overlapping strides", plans, dout.ptr, a2, k2, 3, T, (n, n)),
        ("output is an operand", plans, dout.ptr, [din.ptr, dout.ptr], k2, 3, T | ACC, None),
        ("output is a key", plans, dout.ptr, a2, [dkey.ptr, dout.ptr], 3, T, None),
        ("output is a broadcast key", plans, dout.ptr, a2, [dkey.ptr, dout.ptr + 8 * (words - n)], 3, T | BC, None),
    ]
    for what, ps, c, a, key, g, flags, lay in dot:
        with pytest.raises(lib.NttError):
            lib.rns_galois_dot(ps, c, a, key, g, batch, flags, layout=lay)
        untouched(what)
    for p in plans + [other]:
        p.destroy()
    din.free(), dout.free(), dkey.free()


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_rotate")
    got = {(int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))): int(m.group(5), 16)
           for m in re.finditer(r"rotation (\d+) (\w+) poly (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    n, nq, np_, alpha, digits = 1 << 13, 8, 2, 2, 4
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(7)] + [lib.find_prime(60, n, k) for k in (1, 2)]
    roots = [lib.min_root(q, n) for q in primes]
    assert len(got) == 2 * 2 * 2 * nq
    ext = {}
    for p in range(2):
        for k in range(digits):
            e = [np.zeros(n, dtype=np.uint64) for _ in primes]
            for l in range(alpha * k, alpha * (k + 1)):
                e[l] = oracle.fill_uniform(n, primes[l], 100 + 16 * p + l)
            e = km.mod_up(oracle, primes, roots, e, n, alpha * k, alpha, 0)
            ext[(p, k)] = [oracle.ctx(n, q, w).fwd(x) for q, w, x in zip(primes, roots, e)]
    for r_, steps in enumerate((1, -2)):
        g = gm.rotation(n, steps)
        for p in range(2):
            acc = []
            for l, q in enumerate(primes):
                keys = [oracle.fill_uniform(n, q, 1000 + 100 * r_ + 16 * k + l) for k in range(digits)]
                acc.append(gm.dot_model(oracle, None, [ext[(p, k)][l] for k in range(digits)], keys, n, g, q, T | BC))
            out, _ = km.mod_down(oracle, primes, roots, np_, acc, n, km.TRANSFORMED)
            for l in range(nq):
                assert got[(r_, "switched", p, l)] == oracle.checksum(out[l]), (r_, p, l)
                c0 = oracle.fill_uniform(n, primes[l], 200 + 16 * p + l)
                assert got[(r_, "c0", p, l)] == oracle.checksum(gm.ntt_model(c0, n, g)), (r_, p, l)


@pytest.mark.gpu
def test_route_proof_two_launches_for_17_limbs_and_one_for_a_dot_over_16():
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    assert len(launched) == 3, launched
    assert all(k.startswith("galois_ntt_kernel") for k in launched[:2]), launched
    assert launched[2] == "galois_dot_kernel", launched
