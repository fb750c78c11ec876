"""GPU: the device-side sampler (ntt_rns_sample_batch / _strided).  Every output word against the Python model of
tests/sample_model.py, bit for bit: the coefficient route over shapes, limb counts, kinds and accumulation; the 16-limb chunk; batch
splits; the multiplier's corners; threads that wrap; every sample_fwd_kernel instance; the persistent loop's wrap; mixed chains; the
composition at large sizes and for the integer policies; layouts with canaries; fused == composition; the option; argument errors that
write nothing; the plain-C example; and two kernel traces: the route at 2^14 over 17 FP64 limbs (two sample_fwd_kernel launches,
nothing else) and the launch of all 37 new kernels."""
import os

import numpy as np
import pytest

import children
import rns_support as rs
import sample_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "sample_model.py")
T, A = sm.TRANSFORMED, sm.ACCUMULATE
SMALL = [sm.TERNARY, sm.CBD21]
SMALL_IDS = sm.KIND_IDS[:2]


# ---------------------------------------------------------------- the coefficient route

@pytest.mark.gpu
@pytest.mark.parametrize("logn,batch", [(1, 1), (1, 3), (6, 130), (12, 3)])
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_coefficient_shapes(lib, oracle, logn, batch, kind, acc):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 60, 30])
    sm.check_sample(lib, oracle, primes, roots, n, batch, kind, acc, seed=0x5EED + logn, first_poly=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [1, 2, 16, 17, 34])
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_coefficient_limb_counts_across_the_chunk(lib, oracle, nlimbs, kind, acc):
    """the uniform tag continues across the 16-limb chunk (limb 16 is tagged 2 | 16 << 8, not 2 | 0 << 8); the small kinds' centred
    value is the same in every limb"""
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    got = sm.check_sample(lib, oracle, primes, roots, n, 2, kind, acc, first_poly=7)
    if acc:
        return
    if kind == sm.UNIFORM:
        if nlimbs > 16:
            first = sm.uniform(0x5EED, 7, n, 0, primes[16])  # what limb 16 would hold had the tag started again
            assert not np.array_equal(got[16][:n], first)
    else:
        v = sm.centred(got[0], primes[0])
        assert int(np.abs(v).max()) <= 21
        for l in range(1, nlimbs):
            assert np.array_equal(sm.centred(got[l], primes[l]), v), l


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, (1 << 32) - 2, (1 << 64) - 3], ids=["first0", "first2p32m2", "first2p64m3"])
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
@pytest.mark.parametrize("flags", [0, T], ids=["coef", "ntt"])
def test_batch_split_invariance(lib, oracle, first, kind, flags):
    """batch = 5 at first_poly = F equals the calls (2, F) and (3, F + 2) concatenated, across the carries of P at 2^32 and 2^64"""
    n = 1 << 7
    primes, roots = rs.chain(lib, n, [50, 60, 30])
    whole = sm.check_sample(lib, oracle, primes, roots, n, 5, kind, flags, first_poly=first)
    head = sm.check_sample(lib, oracle, primes, roots, n, 2, kind, flags, first_poly=first)
    tail = sm.check_sample(lib, oracle, primes, roots, n, 3, kind, flags, first_poly=(first + 2) % (1 << 64))
    for w, h, t in zip(whole, head, tail):
        assert np.array_equal(w, np.concatenate([h, t]))


@pytest.mark.gpu
@pytest.mark.parametrize("mult", sm.MULTS + [1 << 60, 3 * ((1 << 30) + 3)], ids=["mult1", "mult65537", "mult2p61m1", "mult2p60", "multodd"])
@pytest.mark.parametrize("kind", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("flags", [0, A, T | A])
def test_multiplier_corners(lib, oracle, mult, kind, flags):
    """mult = 1, t, the largest, a power of two and a multiple of nothing in particular; against 60-, 50- and 30-bit primes (mult >= q:
    reduced per limb on the host)"""
    n = 1 << 7
    primes, roots = rs.chain(lib, n, [60, 50, 30])
    sm.check_sample(lib, oracle, primes, roots, n, 2, kind, flags, mult=mult)
    # a multiplier that is a multiple of one of the primes: that limb is all zeros (store) -- still canonical
    sm.check_sample(lib, oracle, primes, roots, n, 2, kind, flags, mult=primes[2] * 5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
def test_coefficient_max_grid(lib, oracle, kind):
    """3 workgroups of 256 threads over 5 * 2^10 positions: every thread wraps six or seven times"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    sm.check_sample(lib, oracle, primes, roots, n, 5, kind, max_grid=3)


# ---------------------------------------------------------------- the fused route

@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn):
    """each sample_fwd_kernel<policy, LOGN, class>: three limbs of the class, batch 3 below 2^9 (a partly dead group of sub-blocks),
    kind, multiplier and accumulation rotating with LOGN, first_poly = 2^32 - 1 (P carries inside the call)"""
    sm.run_instance(lib, oracle, pol, k, logn)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [12, 14])
@pytest.mark.parametrize("batch", [5, 13])
@pytest.mark.parametrize("flags", [T, T | A])
def test_persistent_loop_wrap(lib, oracle, logn, batch, flags):
    """the smallest grid (8 workgroups per limb: the x extent is a multiple of 8): batch 5 leaves workgroups without a block, batch 13
    wraps five of them, the last block served by a wrapped iteration"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    sm.check_sample(lib, oracle, primes, roots, n, batch, sm.CBD21, flags, max_grid=3, fused=1, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [[60, 50, 50, 52, 50, 50], [50, 50, 51, 60], [60, 30]], ids=["60-first", "60-last", "60-30"])
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
@pytest.mark.parametrize("fused", [1, None], ids=["fused", "default"])
def test_mixed_chains(lib, oracle, bits, kind, acc, fused):
    """fused and composed runs in one call; the uniform tag follows the limb's index in the call, not in its run"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, bits)
    sm.check_sample(lib, oracle, primes, roots, n, 3, kind, T | acc, fused=fused, seed=len(bits))


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16, 17])
@pytest.mark.parametrize("kind,flags", [(sm.TERNARY, T), (sm.CBD21, T | A)])
def test_composition_at_large_sizes(lib, oracle, logn, kind, flags):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50])
    sm.check_sample(lib, oracle, primes, roots, n, 2, kind, flags, seed=logn, fused=1)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["u64", "r4"])
@pytest.mark.parametrize("kind", sm.KINDS, ids=sm.KIND_IDS)
@pytest.mark.parametrize("flags", [0, T, T | A])
def test_integer_policy_limbs(lib, oracle, arith, kind, flags):
    n = 1 << 12
    a = {"u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58, 58, 58])
    sm.check_sample(lib, oracle, primes, roots, n, 3, kind, flags, arith=a, seed=7, fused=1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [0, A, T, T | A])
def test_layouts_with_canaries(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50, 52])
    sm.check_sample(lib, oracle, primes, roots, n, 3, sm.CBD21, flags, layout=layout, seed=11, fused=1)
    sm.check_sample(lib, oracle, primes, roots, n, 3, sm.UNIFORM, flags, layout=layout, seed=12)
    sm.check_sample(lib, oracle, primes, roots, n, 3, sm.TERNARY, flags, layout=layout, seed=13, fused=0)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nlimbs", [(14, 17), (9, 5), (12, 20)])
@pytest.mark.parametrize("kind", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_fused_equals_composition_bit_for_bit(lib, oracle, logn, nlimbs, kind, acc):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    kw = dict(seed=3, first_poly=(1 << 64) - 1, mult=65537)
    fused = sm.check_sample(lib, oracle, primes, roots, n, 2, kind, T | acc, fused=1, **kw)
    composed = sm.check_sample(lib, oracle, primes, roots, n, 2, kind, T | acc, fused=0, **kw)
    for a, b in zip(fused, composed):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_uniform_is_the_same_in_either_domain(lib, oracle):
    """NTT_SAMPLE_TRANSFORMED is accepted with the uniform kind and changes nothing, whatever the route option says"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 50, 60])
    plain = sm.check_sample(lib, oracle, primes, roots, n, 2, sm.UNIFORM, 0)
    for fused in (0, 1, None):
        dom = sm.check_sample(lib, oracle, primes, roots, n, 2, sm.UNIFORM, T, fused=fused)
        for a, b in zip(plain, dom):
            assert np.array_equal(a, b)


@pytest.mark.gpu
def test_option_defaults_and_round_trips(lib):
    n = 1 << 8
    q = lib.find_prime(50, n)
    p = lib.Plan(n, q, lib.min_root(q, n))
    assert p.get_option(lib.OPT_SAMPLE_FUSED) == -1
    for v, want in ((1, 1), (0, 0), (7, 1), (-1, -1)):
        p.set_option(lib.OPT_SAMPLE_FUSED, v)
        assert p.get_option(lib.OPT_SAMPLE_FUSED) == want
    p.destroy()


# ---------------------------------------------------------------- argument errors

@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    q2 = lib.find_prime(50, 2 * n)
    other = lib.Plan(2 * n, q2, lib.min_root(q2, 2 * n))
    with pytest.raises(lib.NttError):  # a prime >= 2^61 cannot reach the call: no plan is created for one
        lib.Plan(n, (1 << 61) + 1, 3)
    fwd_only = rs.forward_only_plan(lib, n, primes[2], roots[2])
    img = oracle.fill_uniform(3 * batch * n, min(primes), 5)  # canonical for every limb
    buf = lib.DeviceBuffer(img.size).upload(img)
    c = buf.ptr
    bad = [
        ("unknown kind", plans, c, 3, 1, 0, None),
        ("negative kind", plans, c, -1, 1, 0, None),
        ("unknown flag 1", plans, c, sm.CBD21, 1, 1, None),
        ("unknown flag 8", plans, c, sm.CBD21, 1, 8, None),
        ("mult = 0", plans, c, sm.TERNARY, 0, 0, None),
        ("mult = 2^61", plans, c, sm.TERNARY, 1 << 61, 0, None),
        ("mult != 1 with the uniform kind", plans, c, sm.UNIFORM, 2, 0, None),
        ("differing N", [plans[0], other], c, sm.TERNARY, 1, 0, None),
        ("null output", plans, None, sm.TERNARY, 1, 0, None),
        ("overlapping strides", plans, c, sm.TERNARY, 1, T, (n, n)),
        ("a stride below N", plans, c, sm.UNIFORM, 1, 0, (batch * n, n - 1)),
        ("no inverse table, composed accumulation", plans[:2] + [fwd_only], c, sm.CBD21, 1, T | A, None),
    ]
    plans[0].set_option(lib.OPT_SAMPLE_FUSED, 0)
    for what, ps, dc, kind, mult, flags, lay in bad:
        with pytest.raises(lib.NttError):
            lib.rns_sample(ps, dc, kind, 0x5EED, batch, mult=mult, flags=flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    plans[0].set_option(lib.OPT_SAMPLE_FUSED, -1)
    # the forward table alone serves the fused accumulation and every storing route
    plans[0].set_option(lib.OPT_SAMPLE_FUSED, 1)
    lib.rns_sample(plans[:2] + [fwd_only], c, sm.CBD21, 0x5EED, batch, flags=T | A)
    plans[0].set_option(lib.OPT_SAMPLE_FUSED, -1)
    got = buf.download()  # (waits for the call: nothing is in flight when the plans go)
    per = batch * n
    want = sm.expected(oracle, sm.CBD21, primes, roots, n, batch, 0x5EED, 0, 1, T | A, [img[l * per:(l + 1) * per] for l in range(3)])
    assert np.array_equal(got, np.concatenate(want))
    for p in plans + [other]:
        p.destroy()
    fwd_only.destroy()
    buf.free()


# ---------------------------------------------------------------- the example

@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_sample")
    assert out.splitlines() == sm.example_model(lib, oracle)


# ---------------------------------------------------------------- kernel traces

@pytest.mark.gpu
def test_route_proof_two_fused_launches():
    """2^14, 17 FP64 limbs, NTT domain, the fused kernel selected: the call launches exactly two sample_fwd_kernels, one per run of at
    most 16 limbs, and nothing else"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    assert launched == ["sample_fwd_kernel<ArithF64,14,1>"] * 2, launched


@pytest.mark.gpu
def test_launch_proof_every_new_kernel():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = rs.kernel_names("sample_fwd_kernel", rs.fused_launch_cases()) | {"sample_coef_kernel"}
    assert len(want) == 37
    assert not sorted(want - launched), "kernels never launched: %s" % sorted(want - launched)
