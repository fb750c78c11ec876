"""GPU: the lifts into the RNS (ntt_rns_from_plain_batch, ntt_rns_from_double_batch / _strided).  Every output word against the
big-integer definitions of tests/lift_model.py, bit for bit: the coefficient route over shapes, limb counts, plaintext moduli, modes and
accumulation; every lift_fwd_kernel instance; the persistent loop's wrap; mixed chains; the composition at large sizes and for the
integer policies; layouts with canaries; a broadcast lifted plaintext fed to rns_lincomb; corner words; fused == composition;
argument errors that write nothing; round trips through rns_to_plain / rns_to_double; the plain-C example; and two kernel traces: the
route at 2^14 over 17 FP64 limbs (two lift_fwd_kernel launches, nothing else) and the launch of all 37 new kernels."""
import os
from math import prod

import numpy as np
import pytest

import children
import lift_model as lm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "lift_model.py")
S, T, A = lm.SCALE, lm.TRANSFORMED, lm.ACCUMULATE
GPU_TS = [2, 256, 65537, 1 << 32, (1 << 61) - 1]
MODES = [("plain", 0), ("plain", S), (lm.DOUBLE, 0)]
MODE_IDS = ["centred", "scaled", "double"]


def _arg(kind, t=65537, scale=2.0 ** 40):
    return {"scale": scale} if kind == lm.DOUBLE else {"t": t}


# ---------------------------------------------------------------- the coefficient route

@pytest.mark.gpu
@pytest.mark.parametrize("logn,batch", [(1, 1), (1, 3), (6, 130), (12, 3)])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_coefficient_shapes(lib, oracle, logn, batch, mode, acc):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 60, 30])
    lm.check_lift(lib, oracle, primes, roots, n, batch, mode[0], mode[1] | acc, seed=logn + batch, **_arg(mode[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [1, 2, 16, 17, 34])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_coefficient_limb_counts_across_the_chunk(lib, oracle, nlimbs, mode, acc):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    lm.check_lift(lib, oracle, primes, roots, n, 2, mode[0], mode[1] | acc, seed=nlimbs, **_arg(mode[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("t", GPU_TS)
@pytest.mark.parametrize("flags", [0, S, A, S | A])
def test_coefficient_plaintext_moduli_with_their_corner_words(lib, oracle, t, flags):
    """every t with m in {0, 1, ceil(t/2) - 1, ceil(t/2), t - 1} and, scaled, the constructed ties and boundaries (the generator's
    own test is in test_lift_cpu.py)"""
    n = 1 << 7
    primes, roots = rs.chain(lib, n, [50, 60, 30, 52])
    corners = lm.plain_corners(t, primes if flags & S else None)
    assert {0, 1 % t, t - 1, t - t // 2, (t - t // 2 - 1) % t} <= set(corners)
    lm.check_lift(lib, oracle, primes, roots, n, 2, "plain", flags, t=t, seed=t % 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0, 3.0, 2.0 ** 40, -2.0 ** 60, 2.0 ** -1074])
@pytest.mark.parametrize("flags", [0, T | A])
def test_double_corner_words(lib, oracle, scale, flags):
    """+-0.0, +-0.5, 1.5, 2.5, 2^53 + 2, just below 2^127 and 2^127, NaN, +-inf, the smallest subnormal, products that round"""
    n = 1 << 6
    primes, roots = rs.chain(lib, n, [50, 60, 30])
    words = lm.with_corners(lm.DOUBLE, 2 * n, 0, 9, flags, primes)
    assert lm.double_corners().size <= words.size
    lm.check_lift(lib, oracle, primes, roots, n, 2, lm.DOUBLE, flags, scale=scale, plain=words)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_coefficient_max_grid(lib, oracle, mode):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    lm.check_lift(lib, oracle, primes, roots, n, 5, mode[0], mode[1], max_grid=3, seed=5, **_arg(mode[0]))


# ---------------------------------------------------------------- the fused route

@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn):
    """each lift_fwd_kernel<policy, LOGN, class>: three limbs of the class, batch 3 below 2^9 (a partly dead group of sub-blocks), mode
    and accumulation rotating with LOGN"""
    lm.run_instance(lib, oracle, pol, k, logn)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [12, 14])
@pytest.mark.parametrize("batch", [5, 13])
@pytest.mark.parametrize("flags", [T | S, T | A])
def test_persistent_loop_wrap(lib, oracle, logn, batch, flags):
    """the smallest grid (8 workgroups per limb: the x extent is a multiple of 8): batch 5 leaves workgroups without a block, batch 13
    wraps five of them, the last block served by a wrapped iteration"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    lm.check_lift(lib, oracle, primes, roots, n, batch, "plain", flags, max_grid=3, fused=1, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [[60, 50, 50, 52, 50, 50], [50, 50, 51, 60], [60, 30]], ids=["60-first", "60-last", "60-30"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_mixed_chains(lib, oracle, bits, mode, acc):
    """fused and composed runs in one call"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, bits)
    lm.check_lift(lib, oracle, primes, roots, n, 3, mode[0], T | mode[1] | acc, seed=len(bits), **_arg(mode[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16, 17])
@pytest.mark.parametrize("flags", [T, T | S | A])
def test_composition_at_large_sizes(lib, oracle, logn, flags):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50])
    lm.check_lift(lib, oracle, primes, roots, n, 2, "plain", flags, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["u64", "r4"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("flags", [0, T, T | A])
def test_integer_policy_limbs(lib, oracle, arith, mode, flags):
    n = 1 << 12
    a = {"u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58, 58, 58])
    lm.check_lift(lib, oracle, primes, roots, n, 3, mode[0], flags | mode[1], arith=a, seed=7, **_arg(mode[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [0, A, T, T | S | A])
def test_layouts_and_plaintext_stride(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50, 52])
    lm.check_lift(lib, oracle, primes, roots, n, 3, "plain", flags, layout=layout, m_stride=n + 24, seed=11)
    lm.check_lift(lib, oracle, primes, roots, n, 3, lm.DOUBLE, flags & ~S, layout=layout, m_stride=n + 24, seed=12, scale=2.0 ** 45)


@pytest.mark.gpu
def test_broadcast_lifted_plaintext_multiplies_through_lincomb(lib, oracle):
    """ct (.) pt: pt^ = from_plain(batch = 1, TRANSFORMED) is the [limb][N] multiplier LINCOMB_M_BROADCAST reads"""
    n, batch, t = 1 << 10, 3, 65537
    primes, roots = rs.chain(lib, n, [50, 50, 52])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    m = lm.with_corners("plain", n, t, 3, 0, primes)
    ct = [oracle.fill_uniform(batch * n, q, 40 + l) for l, q in enumerate(primes)]
    dm, dpt = lib.DeviceBuffer(n).upload(m), lib.DeviceBuffer(len(primes) * n)
    dct, dout = lib.DeviceBuffer(len(primes) * batch * n).upload(np.concatenate(ct)), lib.DeviceBuffer(len(primes) * batch * n)
    lib.rns_from_plain(plans, dpt.ptr, dm.ptr, t, 1, T)
    lib.rns_lincomb(plans, dout.ptr, [dct.ptr], dms=[dpt.ptr], batch=batch, flags=lib.LINCOMB_M_BROADCAST)
    got = dout.download()
    pt = lm.expected(oracle, "plain", m, primes, roots, n, T, t)
    for l, q in enumerate(primes):
        want = oracle.pointwise(ct[l], np.tile(pt[l], batch), q)
        assert np.array_equal(got[l * batch * n:(l + 1) * batch * n], want), l
    for b in (dm, dpt, dct, dout):
        b.free()
    for p in plans:
        p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nlimbs", [(14, 17), (9, 5), (12, 20)])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_fused_equals_composition_bit_for_bit(lib, oracle, logn, nlimbs, mode, acc):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    kw = dict(seed=3, **_arg(mode[0]))
    fused = lm.check_lift(lib, oracle, primes, roots, n, 2, mode[0], T | mode[1] | acc, fused=1, **kw)
    composed = lm.check_lift(lib, oracle, primes, roots, n, 2, mode[0], T | mode[1] | acc, fused=0, **kw)
    for a, b in zip(fused, composed):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_option_defaults_and_round_trips(lib):
    n = 1 << 8
    q = lib.find_prime(50, n)
    p = lib.Plan(n, q, lib.min_root(q, n))
    assert p.get_option(lib.OPT_LIFT_FUSED) == -1
    for v, want in ((1, 1), (0, 0), (7, 1), (-1, -1)):
        p.set_option(lib.OPT_LIFT_FUSED, v)
        assert p.get_option(lib.OPT_LIFT_FUSED) == want
    p.destroy()


# ---------------------------------------------------------------- argument errors

@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch, t = 1 << 10, 2, 65537
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    other = lib.Plan(2 * n, lib.find_prime(50, 2 * n), lib.min_root(lib.find_prime(50, 2 * n), 2 * n))
    words = 3 * batch * n
    img = oracle.fill_uniform(words + batch * n, primes[0], 5)
    buf = lib.DeviceBuffer(img.size).upload(img)
    c, m = buf.ptr, buf.ptr + 8 * words
    bad_plain = [
        ("t = 1", plans, c, m, 1, 0, None),
        ("t = 2^61", plans, c, m, 1 << 61, 0, None),
        ("a prime divides t", plans, c, m, 3 * primes[1], S, None),
        ("unknown flag", plans, c, m, t, 8, None),
        ("differing N", [plans[0], other], c, m, t, 0, None),
        ("overlap: the plaintext is limb 0", plans, c, c, t, 0, None),
        ("overlap: the plaintext is the last limb's last polynomial", plans, c, m - 8 * n, t, T, None),
        ("null output", plans, None, m, t, 0, None),
        ("null plaintext", plans, c, None, t, 0, None),
        ("overlapping strides", plans, c, m, t, T, (n, n, n)),
        ("plaintext stride below N", plans, c, m, t, 0, (batch * n, n, n - 1)),
    ]
    for what, ps, dc, dm, tt, flags, lay in bad_plain:
        with pytest.raises(lib.NttError):
            lib.rns_from_plain(ps, dc, dm, tt, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    for what, flags in (("SCALE on from_double", S), ("SCALE | TRANSFORMED on from_double", S | T), ("unknown flag", 16)):
        with pytest.raises(lib.NttError):
            lib.rns_from_double(plans, c, m, 1.0, batch, flags)
        assert np.array_equal(buf.download(), img), what
    for p in plans + [other]:
        p.destroy()
    buf.free()


# ---------------------------------------------------------------- round trips through the shipped calls

@pytest.mark.gpu
@pytest.mark.parametrize("flags_in,flags_out", [(0, 0), (S, 1)], ids=["centred", "scaled"])
@pytest.mark.parametrize("t", [2, 65537, 1 << 32, (1 << 61) - 1])
def test_round_trip_through_to_plain(lib, oracle, t, flags_in, flags_out):
    """rns_to_plain(rns_from_plain(m)) == m.  Q >= 2^20 t: centred, |m_c| <= t / 2 <= 2^-21 Q is far from Q / 2; scaled, t x mod Q for
    x = round(Q m / t) is within t / 2 of 0 or Q -- no word lies in to_plain's band, the definitions alone give the identity"""
    n, batch = 1 << 8, 2
    primes, roots = rs.chain(lib, n, [50, 50])
    assert prod(primes) >= (t << 20) and flags_out == lib.PLAIN_SCALE * (flags_in == S)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    m = lm.with_corners("plain", batch * n, t, 21, flags_in, primes)
    dm, dc, dout = lib.DeviceBuffer(m.size).upload(m), lib.DeviceBuffer(2 * m.size), lib.DeviceBuffer(m.size)
    lib.rns_from_plain(plans, dc.ptr, dm.ptr, t, batch, flags_in)
    lib.rns_to_plain(plans, dout.ptr, dc.ptr, t, batch, flags_out)
    assert np.array_equal(dout.download(), m)
    for b in (dm, dc, dout):
        b.free()
    for p in plans:
        p.destroy()


@pytest.mark.gpu
def test_round_trip_through_to_double(lib, oracle):
    """rns_to_double(rns_from_double(y, Delta), 1 / Delta) == rint(y Delta) / Delta for |y Delta| < 2^53 (Delta a power of two)"""
    n, batch, delta = 1 << 8, 2, 2.0 ** 30
    primes, roots = rs.chain(lib, n, [60, 60])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    rng = np.random.default_rng(8)
    y = rng.standard_normal(batch * n) * np.exp2(rng.integers(-30, 22, size=batch * n))
    y[:6] = [0.0, -0.0, 0.5 / delta, 1.5 / delta, -2.5 / delta, (2.0 ** 53 - 1) / delta]
    assert np.all(np.abs(y * delta) < 2.0 ** 53)
    dy, dc, dout = lib.DeviceBuffer(y.size).upload(y.view(np.uint64)), lib.DeviceBuffer(2 * y.size), lib.DeviceBuffer(y.size)
    lib.rns_from_double(plans, dc.ptr, dy.ptr, delta, batch)
    lib.rns_to_double(plans, dout.ptr, dc.ptr, 1.0 / delta, batch)
    got = dout.download().view(np.float64)
    assert np.array_equal(got, np.rint(y * delta) / delta)
    for b in (dy, dc, dout):
        b.free()
    for p in plans:
        p.destroy()


# ---------------------------------------------------------------- the example

@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_encrypt")
    assert out.splitlines() == lm.example_model(lib, oracle)


# ---------------------------------------------------------------- kernel traces

@pytest.mark.gpu
def test_route_proof_two_fused_launches():
    """2^14, 17 FP64 limbs, NTT domain, the fused kernel selected (the measured default composes a storing centred lift at 2^14): the
    call launches exactly two lift_fwd_kernels, one per run of at most 16 limbs, and nothing else"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    assert launched == ["lift_fwd_kernel<ArithF64,14,1>"] * 2, launched


@pytest.mark.gpu
def test_launch_proof_every_new_kernel():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = rs.kernel_names("lift_fwd_kernel", rs.fused_launch_cases()) | {"lift_coef_kernel"}
    assert len(want) == 37
    assert not sorted(want - launched), "kernels never launched: %s" % sorted(want - launched)
