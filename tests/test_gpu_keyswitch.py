"""GPU: ModUp / ModDown (ntt_rns_mod_up_batch, ntt_rns_mod_down_batch and their strided forms).  Every output word against the model
of tests/keyswitch_model.py: every moddown_fwd_kernel instance with 1, 2 and 4 P primes, the sandwich route (N >= 2^15, integer-policy
Q limbs), ModUp in both domains with digits at the start, middle and end and across the 16-destination launch boundary, mixed chains,
batches, layouts with canaries, ModDown with one P prime against ntt_rns_rescale_batch bit for bit, fused == sandwich, argument errors
that write nothing, the plain-C example; and two kernel traces: the route at 2^14 over 16 + 2 limbs (the P limbs' inverse, one
moddown_fwd_kernel) and the launch of all 38 new instances."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import children
import kernel_inventory
import keyswitch_model as km
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "keyswitch_model.py")
T, F = km.TRANSFORMED, km.FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [1, 2, 4])
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn, np_):
    """each moddown_fwd_kernel<policy, LOGN, class>: three Q limbs of the class, np 60-bit P limbs, NTT domain, round (even LOGN) /
    floor (odd)"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    primes, roots = rs.chain(lib, n, [b] * 3 + [60] * np_)
    flags = T | (F if logn % 2 else 0)
    km.run_down(lib, oracle, primes, roots, np_, n, 3 if logn < 9 else 2, flags, seed=logn + np_)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16, 17])
@pytest.mark.parametrize("flags", [T, T | F])
def test_sandwich_at_large_sizes(lib, oracle, logn, flags):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60, 60])
    km.run_down(lib, oracle, primes, roots, 2, n, 2, flags, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["auto", "u64", "r4"])
@pytest.mark.parametrize("flags", [0, T, T | F])
def test_integer_policy_limbs(lib, oracle, arith, flags):
    """60-bit (wide integer policy), 58-bit with the reference butterflies, the radix-4 policy: the sandwich (NTT domain) or the
    coefficient kernel; ModUp beside it"""
    n = 1 << 12
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58] * 5 if arith != "auto" else [60] * 5)
    plans = [lib.Plan(n, q, w, arith=a) for q, w in zip(primes, roots)]
    try:
        km.run_down(lib, oracle, primes, roots, 2, n, 3, flags, plans=plans, seed=7)
        km.run_up(lib, oracle, primes, roots, 1, 2, n, 3, flags & T, plans=plans, seed=8)
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs,first,count", [(6, 0, 2), (6, 2, 2), (6, 4, 2), (5, 2, 1), (7, 2, 3), (20, 2, 16), (17, 0, 1),
                                                (17, 16, 1), (18, 8, 2), (34, 16, 3), (34, 0, 16), (34, 18, 16)])
@pytest.mark.parametrize("flags", [0, T])
def test_mod_up(lib, oracle, nlimbs, first, count, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 3) + [60, 60])
    km.run_up(lib, oracle, primes, roots, first, count, n, 2, flags, seed=nlimbs + first)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [5, 17, 18, 34])
@pytest.mark.parametrize("flags", [0, T])
def test_mod_down_q_counts_across_the_run_boundary(lib, oracle, nq, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * nq + [60, 60, 60])
    km.run_down(lib, oracle, primes, roots, 3, n, 2, flags, seed=nq)


@pytest.mark.gpu
@pytest.mark.parametrize("qbits,pbits", [([60, 50, 50, 52, 50, 30], [60, 60]), ([52, 52, 50], [60]), ([50, 50, 51], [52, 52, 52]),
                                         ([60, 30], [50, 50]), ([30, 30, 30, 30], [52] * 16)],
                         ids=["60-50-52-30", "52-bit", "p52", "60-30", "p16"])
@pytest.mark.parametrize("flags", [0, F, T, T | F])
def test_mixed_chains(lib, oracle, qbits, pbits, flags):
    n = 1 << 12
    primes, roots = rs.chain(lib, n, qbits + pbits)
    km.run_down(lib, oracle, primes, roots, len(pbits), n, 3, flags, seed=len(qbits))
    if len(pbits) <= 3:
        km.run_up(lib, oracle, primes, roots, 0, 2, n, 3, flags & T, seed=len(qbits))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 130])
@pytest.mark.parametrize("flags", [0, T])
def test_batches(lib, oracle, batch, flags):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50, 60, 60])
    km.run_down(lib, oracle, primes, roots, 2, n, batch, flags, seed=batch)
    km.run_up(lib, oracle, primes, roots, 2, 2, n, batch, flags, seed=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [0, T, T | F])
def test_layouts(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    km.run_down(lib, oracle, primes, roots, 2, n, 3, flags, layout=layout, seed=11)
    km.run_up(lib, oracle, primes, roots, 1, 2, n, 3, flags & T, layout=layout, seed=12)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,bits", [(12, [50] * 5), (12, [60, 50, 50, 52, 50]), (14, [50] * 17), (16, [50, 50, 60])],
                         ids=["2p12-50", "2p12-mixed", "2p14-17", "2p16"])
@pytest.mark.parametrize("flags", [0, F, T, T | F])
def test_mod_down_with_one_p_prime_equals_the_rescale(lib, oracle, logn, bits, flags):
    """ntt_rns_mod_down_batch(nq = L, np = 1) and ntt_rns_rescale_batch(L + 1) on the same operand: the same words"""
    n, batch = 1 << logn, 2
    primes, roots = rs.chain(lib, n, bits)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    coef = [oracle.fill_uniform(batch * n, q, 40 + l) for l, q in enumerate(primes)]
    limbs = [oracle.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    img = np.concatenate(limbs)
    a, b = lib.DeviceBuffer(img.size).upload(img), lib.DeviceBuffer(img.size).upload(img)
    try:
        lib.rns_mod_down(plans, 1, a.ptr, batch, flags)
        lib.rns_rescale(plans, b.ptr, batch, flags)
        assert np.array_equal(a.download(), b.download())
    finally:
        a.free(), b.free()
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nq,np_", [(14, 16, 2), (9, 5, 1), (12, 20, 3), (13, 8, 4)])
def test_fused_equals_sandwich_bit_for_bit(lib, oracle, logn, nq, np_):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * np_)
    fused = km.run_down(lib, oracle, primes, roots, np_, n, 2, T, fused=1, seed=3)
    sandwich = km.run_down(lib, oracle, primes, roots, np_, n, 2, T, fused=0, seed=3)
    for a, b in zip(fused, sandwich):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50] * 18)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    other = lib.Plan(2 * n, lib.find_prime(50, 2 * n), lib.min_root(lib.find_prime(50, 2 * n), 2 * n))
    same = lib.Plan(n, primes[0], roots[0])
    fwd_only = rs.forward_only_plan(lib, n, primes[3], roots[3])
    words = 18 * batch * n
    img = oracle.fill_uniform(words, primes[0], 5)
    buf = lib.DeviceBuffer(words).upload(img)
    p4 = plans[:4]
    down = [
        ("no Q limb", plans[:2], 2, T, None),
        ("no P limb", plans[:2], 0, T, None),
        ("17 P limbs", plans[:18], 17, 0, None),
        ("differing N", [plans[0], other, plans[2], plans[3]], 2, T, None),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 2, 0, None),
        ("overlapping strides", p4, 2, T, (n, n)),
        ("unknown flag", p4, 2, 4, None),
        ("P limb without its inverse table", [plans[0], plans[1], plans[2], fwd_only], 2, T, None),
    ]
    for what, ps, np_, flags, lay in down:
        with pytest.raises(lib.NttError):
            nq = len(ps) - np_
            if lay:
                lib._check(lib._lib.ntt_rns_mod_down_batch_strided(nq, np_, lib._plan_array(ps), buf.ptr, lay[0], lay[1], batch, flags, None))
            else:
                lib._check(lib._lib.ntt_rns_mod_down_batch(nq, np_, lib._plan_array(ps), buf.ptr, batch, flags, None))
        assert np.array_equal(buf.download(), img), what
    up = [
        ("count 0", p4, 0, 0, 0, None),
        ("count 17", plans[:18], 0, 17, 0, None),
        ("digit past the end", p4, 3, 2, 0, None),
        ("negative first", p4, -1, 2, 0, None),
        ("differing N", [plans[0], other, plans[2], plans[3]], 0, 1, 0, None),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 0, 1, 0, None),
        ("overlapping strides", p4, 0, 1, T, (n, n)),
        ("unknown flag", p4, 0, 1, 2, None),
        ("digit limb without its inverse table", [plans[0], plans[1], plans[2], fwd_only], 3, 1, T, None),
    ]
    for what, ps, first, count, flags, lay in up:
        with pytest.raises(lib.NttError):
            lib.rns_mod_up(ps, buf.ptr, first, count, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    # a Q limb without the inverse table: refused where the sandwich serves it, served by the fused route
    fwd_only_q = rs.forward_only_plan(lib, n, primes[1], roots[1])
    ps = [plans[0], fwd_only_q, plans[2], plans[3]]
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 0)
    with pytest.raises(lib.NttError):
        lib.rns_mod_down(ps, 2, buf.ptr, batch, T)
    assert np.array_equal(buf.download(), img), "sandwich without an inverse table"
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 1)
    km.run_down(lib, oracle, primes[:4], roots[:4], 2, n, batch, T, plans=ps, seed=9)
    for p in plans + [other, same, fwd_only, fwd_only_q]:
        p.destroy()
    buf.free()


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_key_switch")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r"poly (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    n, nq, np_, alpha = 1 << 13, 8, 2, 2
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(7)] + [lib.find_prime(60, n, k) for k in (1, 2)]
    roots = [lib.min_root(q, n) for q in primes]
    assert len(got) == 2 * nq
    for p in range(2):
        acc = [np.zeros(n, dtype=np.uint64) for _ in primes]
        for k in range(4):
            ext = [np.zeros(n, dtype=np.uint64) for _ in primes]
            for l in range(alpha * k, alpha * (k + 1)):
                ext[l] = oracle.fill_uniform(n, primes[l], 100 + 16 * p + l)
            ext = km.mod_up(oracle, primes, roots, ext, n, alpha * k, alpha, 0)
            for l, (q, w) in enumerate(zip(primes, roots)):
                key = oracle.fill_uniform(n, q, 1000 + 16 * k + l)
                acc[l] = (acc[l] + oracle.pointwise(oracle.ctx(n, q, w).fwd(ext[l]), key, q)) % np.uint64(q)
        out, _ = km.mod_down(oracle, primes, roots, np_, acc, n, T)
        for l in range(nq):
            assert got[(p, l)] == oracle.checksum(out[l]), (p, l)


@pytest.mark.gpu
def test_route_proof_p_inverses_and_one_fused_launch():
    """2^14, 16 Q limbs of 50-bit primes and 2 P limbs of 60-bit primes, NTT domain: the call launches the inverse transforms of the
    P limbs and exactly one moddown_fwd_kernel, nothing else"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    fused = [k for k in launched if k.startswith("moddown_fwd_kernel")]
    assert fused == ["moddown_fwd_kernel<ArithF64,14,1>"], launched
    others = [k for k in launched if not k.startswith("moddown_fwd_kernel")]
    assert others and all(kernel_inventory.parse(k).args.get("INV") is True for k in others), launched
    assert launched[-1] == fused[0], launched


@pytest.mark.gpu
def test_launch_proof_every_new_instance():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = rs.kernel_names("moddown_fwd_kernel", rs.fused_launch_cases()) | {"moddown_coef_kernel", "bconv_kernel"}
    assert len(want) == 38
    assert not sorted(want - launched), "instances never launched: %s" % sorted(want - launched)
