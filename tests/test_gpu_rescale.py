"""GPU: the RNS rescale (ntt_rns_rescale_batch / _strided).  Every output word against the model of tests/rescale_model.py (small
cases also against round / floor(x / q_L) over the CRT): both domains, round and floor, every rescale_fwd_kernel instance, the
sandwich route (N >= 2^15, integer-policy limbs), runs across the 16-limb boundary, mixed chains, batches, layouts with canaries,
the dropped limb's slot, argument errors that write nothing, fused == sandwich bit for bit, the plain-C example; and two kernel
traces: the route at 2^14 over 17 FP64 limbs (one inverse, one rescale_fwd_kernel) and the launch of all 37 new instances."""
import os
import re

import numpy as np
import pytest

import children
import rescale_model as rm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "rescale_model.py")
T, F = rm.TRANSFORMED, rm.FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn):
    """each rescale_fwd_kernel<policy, LOGN, class>: three limbs of the class, NTT domain, round (even LOGN) / floor (odd)"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [rs.CLASS_BITS[(pol, k)]] * 3)
    flags = T | (F if logn % 2 else 0)
    rm.run_case(lib, oracle, primes, roots, n, 3 if logn < 9 else 2, flags, seed=logn, crt=logn <= 7)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16, 17])
@pytest.mark.parametrize("flags", [T, T | F])
def test_sandwich_at_large_sizes(lib, oracle, logn, flags):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50])
    rm.run_case(lib, oracle, primes, roots, n, 2, flags, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["auto", "u64", "r4"])
@pytest.mark.parametrize("flags", [0, T, T | F])
def test_integer_policy_limbs(lib, oracle, arith, flags):
    """60-bit (wide integer policy), 58-bit with the reference butterflies, the radix-4 policy: the sandwich (NTT domain) or the
    coefficient kernel"""
    n = 1 << 12
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58, 58, 58] if arith != "auto" else [60, 60, 60])
    plans = [lib.Plan(n, q, w, arith=a) for q, w in zip(primes, roots)]
    rm.run_case(lib, oracle, primes, roots, n, 3, flags, plans=plans, seed=7)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [2, 5, 17, 18, 34])
@pytest.mark.parametrize("flags", [0, T])
def test_limb_counts_across_the_run_boundary(lib, oracle, nlimbs, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    rm.run_case(lib, oracle, primes, roots, n, 2, flags, seed=nlimbs, crt=nlimbs <= 5)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [[60, 50, 50, 52, 50, 50], [50, 50, 51, 60], [52, 52, 50], [60, 30]],
                         ids=["60-first", "60-dropped", "52-bit", "60-30"])
@pytest.mark.parametrize("flags", [0, F, T, T | F])
def test_mixed_chains(lib, oracle, bits, flags):
    n = 1 << 12
    primes, roots = rs.chain(lib, n, bits)
    rm.run_case(lib, oracle, primes, roots, n, 3, flags, seed=len(bits), crt=False)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 130])
@pytest.mark.parametrize("flags", [0, T])
def test_batches(lib, oracle, batch, flags):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50, 50])
    rm.run_case(lib, oracle, primes, roots, n, batch, flags, seed=batch, crt=batch <= 3)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [0, T, T | F])
def test_layouts(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 50, 52])
    rm.run_case(lib, oracle, primes, roots, n, 3, flags, layout=layout, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nlimbs", [(14, 17), (9, 5), (12, 20)])
def test_fused_equals_sandwich_bit_for_bit(lib, oracle, logn, nlimbs):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    fused = rm.run_case(lib, oracle, primes, roots, n, 2, T, fused=1, seed=3)
    sandwich = rm.run_case(lib, oracle, primes, roots, n, 2, T, fused=0, seed=3)
    for a, b in zip(fused, sandwich):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    other = lib.Plan(2 * n, lib.find_prime(50, 2 * n), lib.min_root(lib.find_prime(50, 2 * n), 2 * n))
    same = lib.Plan(n, primes[0], roots[0])
    fwd_only = rs.forward_only_plan(lib, n, primes[2], roots[2])
    fwd_only_kept = rs.forward_only_plan(lib, n, primes[1], roots[1])
    words = 3 * batch * n
    img = oracle.fill_uniform(words, primes[0], 5)
    buf = lib.DeviceBuffer(words).upload(img)
    bad = [
        ("one limb", plans[:1], T, None),
        ("differing N", [plans[0], other, plans[2]], T, None),
        ("q_L equal to a kept prime", [plans[0], plans[1], same], 0, None),
        ("overlapping strides", plans, T, (n, n)),
        ("unknown flag", plans, 4, None),
        ("dropped limb without its inverse table", [plans[0], plans[1], fwd_only], T, None),
    ]
    for what, ps, flags, lay in bad:
        with pytest.raises(lib.NttError):
            lib.rns_rescale(ps, buf.ptr, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    # a kept limb without the inverse table: refused where the sandwich serves it, served by the fused route
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 0)
    with pytest.raises(lib.NttError):
        lib.rns_rescale([plans[0], fwd_only_kept, plans[2]], buf.ptr, batch, T)
    assert np.array_equal(buf.download(), img), "sandwich without an inverse table"
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 1)
    assert plans[0].get_option(lib.OPT_RESCALE_FUSED) == 1
    rm.run_case(lib, oracle, primes, roots, n, batch, T, plans=[plans[0], fwd_only_kept, plans[2]], seed=9)
    for p in plans + [other, same, fwd_only, fwd_only_kept]:
        p.destroy()
    buf.free()


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_rescale")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r"poly (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    n = 1 << 13
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(5)]
    roots = [lib.min_root(q, n) for q in primes]
    assert len(got) == 2 * 4
    for p in range(2):
        hats = [oracle.ctx(n, q, w).fwd(oracle.fill_uniform(n, q, 100 + p)) for q, w in zip(primes, roots)]
        once, _ = rm.model(oracle, primes, roots, hats, n, T)
        twice, _ = rm.model(oracle, primes[:-1], roots[:-1], once, n, T)
        for l in range(4):
            assert got[(p, l)] == oracle.checksum(twice[l]), (p, l)


@pytest.mark.gpu
def test_route_proof_one_inverse_and_one_fused_launch():
    """2^14, 17 FP64 limbs (16 kept: one run), NTT domain: the call launches one inverse transform and one rescale_fwd_kernel"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    assert len(launched) == 2, launched
    assert launched[0].startswith("fused_kernel<ArithF64,14,true"), launched
    assert launched[1] == "rescale_fwd_kernel<ArithF64,14,1>", launched


@pytest.mark.gpu
def test_launch_proof_every_new_instance():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = rs.kernel_names("rescale_fwd_kernel", rs.fused_launch_cases()) | {"rescale_coef_kernel"}
    assert len(want) == 37
    assert not sorted(want - launched), "instances never launched: %s" % sorted(want - launched)
