"""GPU: ntt_rns_to_plain_batch and ntt_rns_to_double_batch -- out of the RNS.  Every output word is compared with the formula model of
tests/plain_model.py (to_double: with the correctly rounded conversion of the CRT integer) bit for bit; the operands and the output sit
among canaries, which stay untouched, as the inputs do.  The corner words are also compared with the big-integer definitions wherever
they lie outside the band, and the toy BFV and BGV of the earlier rounds decrypt through the two calls."""
import random
from math import prod

import numpy as np
import pytest

import bgv_model as bm
import children
import exact_bconv_model as xm
import keyswitch_model as km
import plain_model as pm
import rns_support as rs

TS = [2, 256, 65537, 1 << 32, (1 << 61) - 1]
MODES = [0, pm.SCALE]
MODE_IDS = ["centred", "scale"]


def _bits(nlimbs):
    """mixed 60 / 50 / 30-bit primes, the 60-bit one first"""
    return ([60, 50, 30] * 6)[:nlimbs]


# ---------------------------------------------------------------- shapes

@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("nlimbs", [1, 2, 4, 16])
@pytest.mark.parametrize("logn,batch", [(1, 1), (1, 3), (6, 130), (12, 3)])
def test_shapes(lib, logn, batch, nlimbs, t, flags):
    """one limb, the tail groups of one and two, one full group of four loads, four of them; N = 2, one and several workgroups"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, _bits(nlimbs))
    pm.check_plain(lib, primes, roots, n, batch, t, flags, pm.random_limbs(primes, batch * n, logn + batch + nlimbs))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nlimbs", [3, 5, 7, 8, 15])
def test_load_groups_and_tails(lib, nlimbs, flags):
    """every remainder of the groups of four beside the counts of test_shapes"""
    n = 64
    primes, roots = rs.chain(lib, n, _bits(nlimbs))
    pm.check_plain(lib, primes, roots, n, 3, 65537, flags, pm.random_limbs(primes, 3 * n, nlimbs))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
def test_grid_wrap(lib, flags):
    """NTT_OPT_MAX_GRID = 3 on plans[0] at 2^10, 5 polynomials: every thread walks several iterations and polynomials"""
    n, batch = 1 << 10, 5
    primes, roots = rs.chain(lib, n, _bits(5))
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    plans[0].set_option(lib.OPT_MAX_GRID, 3)
    try:
        pm.check_plain(lib, primes, roots, n, batch, 65537, flags, pm.random_limbs(primes, batch * n, 7), plans=plans)
    finally:
        for p in plans:
            p.destroy()


# ---------------------------------------------------------------- layouts, aliasing

@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ["batch_padded", "limb_padded"])
def test_strided(lib, kind, flags):
    """[batch][limb][N] and [limb][batch][N] with padded strides, the output's polynomials N + 24 words apart"""
    n, batch, nl = 64, 5, 6
    primes, roots = rs.chain(lib, n, _bits(nl))
    ls, ps, _ = rs.layout_strides(kind, n, nl, batch)
    pm.check_plain(lib, primes, roots, n, batch, 1 << 32, flags, pm.random_limbs(primes, batch * n, 11), layout=(ls, ps, n + 24))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ["limb", "batch_padded"])
def test_output_in_place_of_limb_0(lib, kind, flags):
    """d_m == d_a: the plaintext lands in limb 0's slots, every other limb and every gap untouched"""
    n, batch, nl = 256, 3, 5
    primes, roots = rs.chain(lib, n, _bits(nl))
    ls, ps, _ = rs.layout_strides(kind, n, nl, batch)
    pm.check_plain(lib, primes, roots, n, batch, 65537, flags, pm.random_limbs(primes, batch * n, 13), layout=(ls, ps, ps), alias=True)


# ---------------------------------------------------------------- corner words

@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nlimbs", [1, 2, 4, 16])
def test_corner_words(lib, nlimbs, flags):
    """x in {0, 1, Q - 1, (Q -+ 1) / 2}; SCALE: t x mod Q = (Q -+ 1) / 2 and the x either side of k Q / t, k = 1 and t - 1 -- bit for
    bit against the model, and against the definition wherever they lie outside the band (inside: one of the two neighbours)"""
    n = 16
    primes, roots = rs.chain(lib, n, _bits(nlimbs))
    Q = prod(primes)
    for t in TS:
        xs = pm.corner_values(Q, t, flags)
        xs += [random.Random(t).randrange(Q) for _ in range(n - len(xs))]
        got = pm.check_plain(lib, primes, roots, n, 1, t, flags, pm.to_rns(xs, primes)).tolist()
        for x, w in zip(xs, got):
            if pm.in_band(x, Q, t, flags):
                assert w in pm.neighbours(x, Q, t, flags), (t, x, w)
            else:
                assert w == pm.definition(x, Q, t, flags), (t, x, w)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
def test_largest_sums(lib, flags):
    """16 limbs of 60-bit primes, every digit z_i = q_i - 1, t = 2^61 - 1: the largest 128-bit sum and the largest FP64 sum"""
    n, t = 16, (1 << 61) - 1
    primes, roots = rs.chain(lib, n, [60] * 16)
    c, _, _, _ = pm.constants(primes, t, flags)
    top = [(q - 1) * pow(ci, -1, q) % q for q, ci in zip(primes, c)]
    limbs = pm.random_limbs(primes, n, 3)
    for l in range(16):
        limbs[l][:4] = top[l]
    pm.check_plain(lib, primes, roots, n, 1, t, flags, limbs)


# ---------------------------------------------------------------- to_double

@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2.0 ** -40, 1.0 / 3.0], ids=["2^-40", "third"])
@pytest.mark.parametrize("bits", [[60, 60], [30]], ids=["60_60", "30"])
@pytest.mark.parametrize("logn,batch", [(6, 3), (1, 1), (10, 5)])
def test_to_double(lib, logn, batch, bits, scale):
    """ties to even at 2^53, a tie and a sticky bit at 2^100, zero (+0.0), -+(Q - 1) / 2 and random words: the bit pattern of
    fl(x_c) * scale, x_c by big-integer CRT, fl Python's correctly rounded conversion"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, bits)
    Q = prod(primes)
    rng = random.Random(logn)
    xs = (pm.double_values(Q) + [rng.randrange(Q) for _ in range(batch * n)])[:batch * n] if n > 2 else pm.double_values(Q)[3:5]
    limbs = pm.to_rns(xs, primes)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    if logn == 10:
        plans[0].set_option(lib.OPT_MAX_GRID, 3)
    try:
        got = pm.run_plain(lib, primes, roots, n, batch, None, 0, limbs, plans=plans, double_scale=scale)
    finally:
        for p in plans:
            p.destroy()
    want = pm.double_model(limbs, primes, scale)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    if n > 2:
        assert got[0] == 0, "x_c = 0 must give +0.0"


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True])
def test_to_double_strided(lib, alias):
    n, batch = 64, 3
    primes, roots = rs.chain(lib, n, [60, 50])
    ls, ps, _ = rs.layout_strides("batch_padded", n, 2, batch)
    limbs = pm.random_limbs(primes, batch * n, 5)
    got = pm.run_plain(lib, primes, roots, n, batch, None, 0, limbs, layout=(ls, ps, ps if alias else n + 8), alias=alias, double_scale=0.125)
    assert np.array_equal(got, pm.double_model(limbs, primes, 0.125))


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_buffers_alone(lib):
    """every refusal of the header: NTT_ERR_ARG (-1), nothing written.  (A prime >= 2^61 cannot reach the call: no plan is created for
    one, which is asserted instead.)"""
    n, batch = 64, 2
    primes, roots = rs.chain(lib, n, [50] * 17)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    other_n = lib.Plan(2 * n, *[v[0] for v in rs.chain(lib, 2 * n, [50])])
    t_div = primes[1] * 3  # SCALE: a prime divides t
    img = np.arange(17 * batch * n, dtype=np.uint64)
    da, dm = lib.DeviceBuffer(img.size).upload(img), lib.DeviceBuffer(img.size).upload(img)
    P, D = lib.rns_to_plain, lib.rns_to_double
    bad = [
        lambda: P(plans[:0], dm.ptr, da.ptr, 65537, batch),
        lambda: P(plans, dm.ptr, da.ptr, 65537, batch),                       # 17 limbs
        lambda: P([plans[0], other_n], dm.ptr, da.ptr, 65537, batch),         # mixed N
        lambda: P([plans[0], plans[0]], dm.ptr, da.ptr, 65537, batch),        # a prime twice
        lambda: P(plans[:4], dm.ptr, da.ptr, 1, batch),
        lambda: P(plans[:4], dm.ptr, da.ptr, 0, batch),
        lambda: P(plans[:4], dm.ptr, da.ptr, 1 << 61, batch),
        lambda: P(plans[:4], dm.ptr, da.ptr, t_div, batch, lib.PLAIN_SCALE),
        lambda: P(plans[:4], dm.ptr, da.ptr, 65537, batch, 2),
        lambda: P(plans[:4], dm.ptr, da.ptr, 65537, batch, lib.PLAIN_SCALE | 4),
        lambda: P(plans[:4], None, da.ptr, 65537, batch),
        lambda: P(plans[:4], dm.ptr, None, 65537, batch),
        lambda: P(plans[:4], dm.ptr, da.ptr, 65537, batch, layout=(n, 4 * n, n - 1)),        # output stride below N
        lambda: P(plans[:4], dm.ptr, da.ptr, 65537, batch, layout=(n, n, n)),                # limbs and polynomials overlap
        lambda: P(plans[:4], da.ptr + 8, da.ptr, 65537, batch),                              # shifted overlap
        lambda: P(plans[:4], da.ptr, da.ptr, 65537, batch, layout=(batch * n, n, n + 8)),    # limb 0 with another stride
        lambda: D(plans[:3], dm.ptr, da.ptr, 1.0, batch),
        lambda: D(plans[:0], dm.ptr, da.ptr, 1.0, batch),
        lambda: D([plans[0], other_n], dm.ptr, da.ptr, 1.0, batch),
        lambda: D(plans[:2], None, da.ptr, 1.0, batch),
        lambda: D(plans[:2], da.ptr + 8 * n, da.ptr, 1.0, batch),
    ]
    try:
        for i, call in enumerate(bad):
            with pytest.raises(lib.NttError, match="status -1"):
                call()
            assert np.array_equal(da.download(), img) and np.array_equal(dm.download(), img), i
        # the default mode needs nothing coprime: the same t is served
        P(plans[:4], dm.ptr, da.ptr, t_div, batch)
        assert int(dm.download(batch * n).max()) < t_div and np.array_equal(da.download(), img)
        with pytest.raises(lib.NttError):
            lib.Plan(n, (1 << 61) + 2 * n * 5 + 1, 3)
    finally:
        da.free(), dm.free()
        for p in plans + [other_n]:
            p.destroy()


# ---------------------------------------------------------------- end to end

def _decrypt_on_device(lib, oracle, primes, roots, n, comps_hat, s, t, flags):
    """the two calls: x = sum_i c_i s^i (ntt_rns_inv_dot_batch on (c_i^) and (1^, s^, s^2^, ..), broadcast), then to_plain"""
    nl = len(primes)
    ctx = [oracle.ctx(n, q, w) for q, w in zip(primes, roots)]
    s_hat = [c.fwd(v) for c, v in zip(ctx, km.residues(s, primes))]
    pw = [[np.ones(n, dtype=np.uint64) for _ in primes]]
    for _ in comps_hat[1:]:
        pw.append([oracle.pointwise(a, b, q) for a, b, q in zip(pw[-1], s_hat, primes)])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    bufs = [lib.DeviceBuffer(nl * n).upload(np.concatenate(v)) for v in list(comps_hat) + pw]
    dx, dm = lib.DeviceBuffer(nl * n), lib.DeviceBuffer(n)
    k = len(comps_hat)
    try:
        lib.rns_inv_dot(plans, dx.ptr, [b.ptr for b in bufs[:k]], [b.ptr for b in bufs[k:]], 1, lib.MUL_B_BROADCAST)
        lib.rns_to_plain(plans, dm.ptr, dx.ptr, t, 1, flags)
        return dm.download().tolist()
    finally:
        for b in bufs + [dx, dm]:
            b.free()
        for p in plans:
            p.destroy()


@pytest.mark.gpu
def test_bfv_product_decrypts_through_the_two_calls(lib, oracle):
    """the toy BFV of exact_bconv_model at N = 64: encrypt, the multiplication of examples/rns_bfv_mul.c on the device, then
    ntt_rns_inv_dot_batch + ntt_rns_to_plain_batch(NTT_PLAIN_SCALE) on (d0, d1, d2): the product of the messages"""
    n, nr, nq, t = 64, 3, 2, 65537
    primes, roots = rs.chain(lib, n, [50] * (nr + nq))
    qp, qr = primes[nr:], roots[nr:]
    Q = prod(qp)
    rng = random.Random(64)
    s = xm.bfv_keygen(rng, n)
    m1, m2 = ([rng.randrange(t) for _ in range(n)] for _ in range(2))
    ct = [p for m in (m1, m2) for p in xm.bfv_encrypt(rng, s, m, n, Q, t)]
    ntt = [[oracle.ctx(n, q, w).fwd(c) for q, w, c in zip(qp, qr, km.residues(p, qp))] for p in ct]
    assert _decrypt_on_device(lib, oracle, qp, qr, n, ntt[:2], s, t, lib.PLAIN_SCALE) == m1
    d = xm.bfv_on_device(lib, primes, roots, nr, t, ntt, n)
    assert _decrypt_on_device(lib, oracle, qp, qr, n, [dj[nr:] for dj in d], s, t, lib.PLAIN_SCALE) == xm.negacyclic(m1, m2, n, t)


@pytest.mark.gpu
def test_bgv_product_decrypts_through_the_two_calls(lib, oracle):
    """the toy BGV of bgv_model at N = 64: encrypt, multiply and relinearise on the device, then ntt_rns_inv_dot_batch +
    ntt_rns_to_plain_batch (default mode): the product of the messages; after the modulus switch, that times q_3^-1 mod T"""
    n, nq, npp, T = 64, 4, 2, bm.PT
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * npp)
    rng = random.Random(65)
    bgv = bm.Bgv(oracle, primes, roots, nq, 2, n, T, rng)
    keys = bgv.relin_keys()
    m1, m2 = ([rng.randrange(T) for _ in range(n)] for _ in range(2))
    ct1, ct2 = bgv.encrypt(m1), bgv.encrypt(m2)
    assert _decrypt_on_device(lib, oracle, primes[:nq], roots[:nq], n, list(ct1), bgv.s, T, 0) == m1
    relin, switched = bm.mul_on_device(lib, bgv, ct1, ct2, keys)
    want = bgv.plain_product(m1, m2)
    assert _decrypt_on_device(lib, oracle, primes[:nq], roots[:nq], n, relin, bgv.s, T, 0) == want
    f = pow(primes[nq - 1], -1, T)
    assert _decrypt_on_device(lib, oracle, primes[:nq - 1], roots[:nq - 1], n, switched, bgv.s, T, 0) == [v * f % T for v in want]


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_decrypt")
    assert out.splitlines() == pm.example_model(lib, oracle)
