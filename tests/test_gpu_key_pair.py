"""GPU: the pair key products -- ntt_rns_fwd_mul_pair_batch, ntt_rns_mod_up_mul_pair_batch, ntt_rns_galois_dot_pair_batch and their strided
forms.  Every word of c0^ and c1^ against the model of tests/key_pair_model.py (the existing models applied once per component,
key0 != key1): every modup_mul2_kernel instance through both entry points, the route proof without a profiler (the sentinel in
d_ext's other slots survives the fused route; d_a is unchanged), the loop shapes, digit positions, layouts with canaries, lazy key
words, the composition route (integer policies, N = 2^5, 2^15, 2^16, mixed chains), equality with the single calls, the Galois
pair, argument errors that write nothing, the plain-C example against the model, and one kernel trace."""
import os
import re

import numpy as np
import pytest

import children
import galois_model as gm
import kernel_inventory
import key_pair_model as kp
import keyswitch_model as km
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "key_pair_model.py")
L, B, A = kp.LAZY_IN, kp.BROADCAST, kp.ACCUMULATE
T, GA, GB = gm.TRANSFORMED, gm.ACCUMULATE, gm.KEY_BROADCAST


def _destroy(plans):
    for p in plans:
        p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_instance(lib, oracle, pol, k, logn):
    """each modup_mul2_kernel<policy, LOGN, class>: three limbs of the class and two 60-bit limbs; digits of one and of two FP64
    limbs, and the 60-bit digit feeding the FP64 run (its own run on the composition); accumulate and broadcast each way.  The same
    instance through ntt_rns_fwd_mul_pair_batch over the three FP64 limbs: d_a is left as it was"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    batch = 3 if logn < 9 else 2
    primes, roots = rs.chain(lib, n, [b, b, b, 60, 60])
    plans = rs.plans(lib, n, primes, roots)
    try:
        for (first, count), flags in (((0, 1), 0), ((1, 2), A | B), ((3, 2), B)):
            _, ext, _ = kp.run(lib, oracle, primes, roots, first, count, n, batch, flags, fused=1, seed=logn + first, plans=plans)
            fp64 = [l for l in range(3) if not first <= l < first + count]
            assert [l for l in kp.untouched(ext, first, count) if l < 3] == fp64, "the FP64 run did not take the fused pair kernel"
        for flags in (A, B):
            _, after, a, _ = kp.run_fwd(lib, oracle, primes[:3], roots[:3], n, batch, flags, fused=1, seed=logn + 7, plans=plans[:3])
            for l in range(3):
                assert np.array_equal(after[l], a[l]), "d_a limb %d was written: the fused pair kernel did not serve the call" % l
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nlimbs,first,count", [(14, 17, 0, 1), (9, 6, 2, 3), (12, 20, 15, 3), (13, 18, 2, 16)])
def test_route_proof_by_the_sentinel(lib, oracle, logn, nlimbs, first, count):
    """an all-FP64 chain.  NTT_OPT_PAIR_FUSED 1: the sentinel in every non-digit slot of d_ext survives, the digit is unchanged;
    0: the same c0^, c1^ bit for bit, and no slot of d_ext holds the sentinel any more (the run was transformed in place)"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nlimbs)
    plans = rs.plans(lib, n, primes, roots)
    digit = range(first, first + count)
    try:
        c1, ext1, up = kp.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=1, seed=3, plans=plans)
        assert kp.untouched(ext1, first, count) == [l for l in range(nlimbs) if l not in digit], "a slot of d_ext was written"
        for l in digit:
            assert np.array_equal(ext1[l], up[l]), "digit limb %d changed" % l
        c0, ext0, _ = kp.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=0, seed=3, plans=plans)
        for j in range(2):
            for l in range(nlimbs):
                assert np.array_equal(c0[j][l], c1[j][l]), "c%d^ limb %d: the routes differ" % (j, l)
        assert not kp.untouched(ext0, first, count), "the composition left a slot of d_ext unwritten"
        for l, (q, w) in enumerate(zip(primes, roots)):
            assert np.array_equal(ext0[l], oracle.ctx(n, q, w).fwd(up[l])), "d_ext limb %d is not the transformed ModUp word" % l
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [6, 10, 14])
def test_fwd_mul_pair_routes(lib, oracle, logn):
    """NTT_OPT_PAIR_FUSED 1: d_a unchanged; 0: the same outputs and d_a holds fwd(a); both equal the two single calls"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 52, 50])
    plans = rs.plans(lib, n, primes, roots)
    try:
        c1, after1, a, fa = kp.run_fwd(lib, oracle, primes, roots, n, 3, A | B, fused=1, seed=4, plans=plans, single=True)
        c0, after0, _, _ = kp.run_fwd(lib, oracle, primes, roots, n, 3, A | B, fused=0, seed=4, plans=plans, single=True)
        for l in range(4):
            assert np.array_equal(after1[l], a[l]), "d_a limb %d changed under the fused kernel" % l
            assert np.array_equal(after0[l], fa[l]), "d_a limb %d is not fwd(a) after the composition" % l
            for j in range(2):
                assert np.array_equal(c0[j][l], c1[j][l])
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,first,count", [([50, 60, 60], 1, 2), ([50, 50], 0, 1)], ids=["two-workgroups", "one-workgroup-per-limb"])
def test_grid_stride_loop_wraps(lib, oracle, bits, first, count):
    """2^14, 5 polynomials, NTT_OPT_MAX_GRID 2: two workgroups for the one FP64 limb (rounds of 2, 2 and 1 blocks), or one per limb"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, bits)
    kp.run(lib, oracle, primes, roots, first, count, n, 5, A | B, fused=1, seed=14, max_grid=2)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,batch", [(8, 73), (8, 1), (10, 130), (6, 5)])
def test_batches(lib, oracle, logn, batch):
    """several blocks per workgroup with the last group partly dead (2^8: 73), one polynomial, 130"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60])
    kp.run(lib, oracle, primes, roots, 1, 2, n, batch, A, fused=1, seed=batch)
    kp.run(lib, oracle, primes, roots, 3, 1, n, batch, B, fused=1, seed=batch + 1)
    kp.run_fwd(lib, oracle, primes[:3], roots[:3], n, batch, A | B, fused=1, seed=batch + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs,first,count", [(6, 0, 2), (6, 2, 2), (6, 4, 2), (5, 2, 1), (20, 2, 16), (17, 0, 1), (17, 16, 1), (34, 16, 3),
                                                (34, 18, 16), (34, 0, 16)])
@pytest.mark.parametrize("fused", [1, -1])
def test_digit_positions(lib, oracle, nlimbs, first, count, fused):
    """digits at the start, in the middle and at the end (inside P), of 1 and of 16 limbs, chains of more than 16 limbs"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 3) + [60, 60])
    kp.run(lib, oracle, primes, roots, first, count, n, 2, A | B, fused=fused, seed=nlimbs + first)


@pytest.mark.gpu
def test_digit_of_largest_words(lib, oracle):
    """every digit word b_i - 1 over 16 limbs: the largest 128-bit sum"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * 18)
    kp.run(lib, oracle, primes, roots, 1, 16, n, 2, A, fused=1, seed=5, digit_max=True)
    primes, roots = rs.chain(lib, n, [60] * 16 + [50, 52])
    kp.run(lib, oracle, primes, roots, 0, 16, n, 2, B, fused=1, seed=6, digit_max=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded"])
@pytest.mark.parametrize("flags", [A, B, A | B])
def test_layouts(lib, oracle, layout, flags):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    kp.run(lib, oracle, primes, roots, 1, 2, n, 3, flags, layout=layout, fused=1, seed=11)
    kp.run_fwd(lib, oracle, primes, roots, n, 3, flags, layout=layout, fused=1, seed=12)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("flags", [L, L | A | B])
def test_lazy_key_words(lib, oracle, flags, fused):
    """key words up to min(4q, 2^53) - 1"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 51, 30, 52, 50])
    kp.run(lib, oracle, primes, roots, 0, 1, n, 3, flags, fused=fused, seed=21, single=True)
    kp.run_fwd(lib, oracle, primes, roots, n, 3, flags, fused=fused, seed=22, single=True)


@pytest.mark.gpu
@pytest.mark.parametrize("arith,bits", [("auto", 60), ("u64", 60), ("r4", 60), ("u64", 57), ("r4", 57)])
def test_composition_integer_policies(lib, oracle, arith, bits):
    """integer-policy plans for a run of 60-bit primes and of 57-bit primes: every run on the composition, whatever NTT_OPT_PAIR_FUSED
    says"""
    n = 1 << 12
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [bits] * 5)
    plans = rs.plans(lib, n, primes, roots, a)
    try:
        _, ext, _ = kp.run(lib, oracle, primes, roots, 1, 2, n, 3, A | B, fused=1, seed=7, plans=plans, single=True)
        assert not kp.untouched(ext, 1, 2), "an integer-policy run cannot take the fused kernel"
        kp.run(lib, oracle, primes, roots, 4, 1, n, 3, 0, fused=1, seed=8, plans=plans)
        _, after, _, fa = kp.run_fwd(lib, oracle, primes, roots, n, 3, A, fused=1, seed=9, plans=plans, single=True)
        for l in range(5):
            assert np.array_equal(after[l], fa[l])
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [5, 15, 16])
def test_composition_outside_the_fused_sizes(lib, oracle, logn):
    """N = 2^5, and 2^15 / 2^16 at batch 2 where the single call uses the operand as scratch: the second component is formed from the
    one transform, not from a transform of overwritten data"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60, 60])
    _, ext, _ = kp.run(lib, oracle, primes, roots, 1, 2, n, 2, A | B, fused=1, seed=logn)
    assert not kp.untouched(ext, 1, 2)
    kp.run(lib, oracle, primes, roots, 3, 2, n, 2, 0, fused=1, seed=logn + 1)
    kp.run_fwd(lib, oracle, primes, roots, n, 2, B, fused=1, seed=logn + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0, -1])
@pytest.mark.parametrize("first,count", [(0, 2), (2, 3), (6, 2)])
def test_mixed_chains(lib, oracle, first, count, fused):
    """a 60-bit first prime, 50-bit (and 52-, 30-bit) primes behind it, a 60-bit P"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, [60, 50, 50, 52, 50, 30] + [60, 60])
    kp.run(lib, oracle, primes, roots, first, count, n, 3, A | B, fused=fused, seed=first, single=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 4, 5, 32])
@pytest.mark.parametrize("flags", [T, T | GA, T | GB, T | GA | GB], ids=["plain", "acc", "bcast", "acc-bcast"])
def test_galois_pair(lib, oracle, k, flags):
    """k across the four-at-a-time loop and its tail; a rotation by 1, by -3, the conjugation and the identity; 57- and 60-bit primes"""
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 57, 60])
    plans = rs.plans(lib, n, primes, roots)
    try:
        for i, g in enumerate((gm.rotation(n, 1), gm.rotation(n, -3), 2 * n - 1, 1)):
            if k == 32 and i > 1:
                continue
            kp.run_dot(lib, oracle, primes, roots, n, 2, k, g, flags, seed=k + i, plans=plans, single=(i == 0))
    finally:
        _destroy(plans)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch_padded"])
def test_galois_pair_sizes_limb_counts_and_extremes(lib, oracle, layout):
    """N = 2^4; 17 limbs (two launches) at 2^11; 32 products of q - 1 words on top of c = q - 1"""
    primes, roots = rs.chain(lib, 16, [60, 57, 50])
    kp.run_dot(lib, oracle, primes, roots, 16, 3, 3, gm.rotation(16, -3), T | GA, layout=layout, seed=2, single=True)
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [60] + [50] * 16)
    kp.run_dot(lib, oracle, primes, roots, n, 2, 3, gm.rotation(n, 1), T | GA | GB, layout=layout, seed=3, single=True)
    primes, roots = rs.chain(lib, n, [60, 57])
    kp.run_dot(lib, oracle, primes, roots, n, 2, 32, 2 * n - 1, T | GA, layout=layout, seed=4, extreme=True)


@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50] * 18)
    plans = rs.plans(lib, n, primes, roots)
    words = 18 * batch * n
    imgs = [oracle.fill_uniform(words, primes[0], 5 + i) for i in range(5)]
    dc0, dc1, dext, dk0, dk1 = bufs = [lib.DeviceBuffer(words).upload(i) for i in imgs]
    p4 = plans[:4]
    four = 4 * batch * n
    inside = 8 * (four - 1)
    bad = [
        ("count 0", p4, 0, 0, 0, {}),
        ("count 17", plans, 0, 17, 0, {}),
        ("digit past the end", p4, 3, 2, 0, {}),
        ("unknown flag", p4, 0, 1, 8, {}),
        ("null c0", p4, 0, 1, 0, {"c0": None}),
        ("null c1", p4, 0, 1, 0, {"c1": None}),
        ("null ext", p4, 0, 1, 0, {"x": None}),
        ("null key0", p4, 0, 1, 0, {"k0": None}),
        ("null key1", p4, 0, 1, 0, {"k1": None}),
        ("c0 is c1", p4, 0, 1, 0, {"c1": dc0.ptr}),
        ("c1 starts inside c0", p4, 0, 1, 0, {"c1": dc0.ptr + inside}),
        ("c0 is the operand", p4, 0, 1, A, {"c0": dext.ptr}),
        ("c1 starts inside the operand", p4, 0, 1, 0, {"c1": dext.ptr + inside}),
        ("c0 is key1", p4, 0, 1, 0, {"c0": dk1.ptr}),
        ("c1 starts inside key0", p4, 0, 1, 0, {"c1": dk0.ptr + inside}),
    ]
    try:
        for fused in (1, 0):
            plans[0].set_option(lib.OPT_PAIR_FUSED, fused)
            for what, ps, first, count, flags, ptr in bad:
                args = [ptr.get(k, d.ptr) for k, d in (("c0", dc0), ("c1", dc1), ("x", dext), ("k0", dk0), ("k1", dk1))]
                with pytest.raises(lib.NttError):
                    lib.rns_mod_up_mul_pair(ps, args[0], args[1], args[2], first, count, args[3], args[4], batch, flags)
                if count == 1:  # the same pointers and flags through fwd_mul_pair
                    with pytest.raises(lib.NttError):
                        lib.rns_fwd_mul_pair(ps, args[0], args[1], args[2], args[3], args[4], batch, flags)
                for buf, img in zip(bufs, imgs):
                    assert np.array_equal(buf.download(), img), what
            # the Galois pair: an output against the other output, an input, a key of either component; a null key list; an even g
            g = gm.rotation(n, 1)
            for what, c0, c1, a, k0, k1, gg, flags in [
                    ("outputs overlap", dc0.ptr, dc0.ptr + inside, [dext.ptr], [dk0.ptr], [dk1.ptr], g, T),
                    ("c1 is an input", dc0.ptr, dext.ptr, [dext.ptr], [dk0.ptr], [dk1.ptr], g, T),
                    ("c0 is a key of component 1", dk1.ptr, dc1.ptr, [dext.ptr], [dk0.ptr], [dk1.ptr], g, T),
                    ("c1 is a key of component 0", dc0.ptr, dk0.ptr, [dext.ptr], [dk0.ptr], [dk1.ptr], g, T),
                    ("null key", dc0.ptr, dc1.ptr, [dext.ptr], [dk0.ptr], [None], g, T),
                    ("null c1", dc0.ptr, None, [dext.ptr], [dk0.ptr], [dk1.ptr], g, T),
                    ("even g", dc0.ptr, dc1.ptr, [dext.ptr], [dk0.ptr], [dk1.ptr], 2, T),
                    ("unknown flag", dc0.ptr, dc1.ptr, [dext.ptr], [dk0.ptr], [dk1.ptr], g, 8)]:
                with pytest.raises(lib.NttError):
                    lib.rns_galois_dot_pair(p4, c0, c1, a, k0, k1, gg, batch, flags)
                for buf, img in zip(bufs, imgs):
                    assert np.array_equal(buf.download(), img), what
        # c1^ right behind c0^'s last word is no overlap; c_j^ may alias its own key (ntt_rns_fwd_mul_batch's rule)
        plans[0].set_option(lib.OPT_PAIR_FUSED, 1)
        lib.rns_mod_up_mul_pair(p4, dc0.ptr, dc0.ptr + 8 * four, dext.ptr, 0, 1, dk0.ptr, dk1.ptr, batch, 0)
        lib.rns_mod_up_mul_pair(p4, dk0.ptr, dk1.ptr, dext.ptr, 0, 1, dk0.ptr, dk1.ptr, batch, 0)
    finally:
        for d in bufs:
            d.free()
        _destroy(plans)


@pytest.mark.gpu
def test_pair_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_key_switch_pair")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in (re.match(r"comp (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", line) for line in out.splitlines()) if m}
    assert len(got) == 16
    n, nq, np_, alpha = 1 << 13, 8, 2, 2
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(7)] + [lib.find_prime(60, n, k) for k in (1, 2)]
    roots = [lib.min_root(q, n) for q in primes]
    accs = [[np.zeros(n, dtype=np.uint64) for _ in primes] for _ in range(2)]
    for k in range(4):
        digit = [oracle.fill_uniform(n, primes[l], 100 + l) for l in range(alpha * k, alpha * (k + 1))]
        keys = [[oracle.fill_uniform(n, q, base + 16 * k + l) for l, q in enumerate(primes)] for base in (1000, 2000)]
        accs, _ = kp.model(oracle, primes, roots, digit, keys, accs, n, 1, alpha * k, alpha, A | B)
    for j in range(2):
        out, _ = km.mod_down(oracle, primes, roots, np_, accs[j], n, km.TRANSFORMED)
        for l in range(nq):
            assert got[(j, l)] == oracle.checksum(out[l]), (j, l)
    assert got[(0, 0)] != got[(1, 0)]


@pytest.mark.gpu
def test_launch_proof_every_instance_and_the_route_call():
    """one traced child (tests/key_pair_model.py; tracing only, no counters): all 36 instances launched; the route call (2^14, 16 x
    50-bit + 2 x 60-bit, digit (0, 2), NTT_OPT_PAIR_FUSED 1) is the only launch of modup_mul2_kernel<ArithF64,14,1> -- ONE fused launch
    for the FP64 run --, no single-component product kernel runs anywhere in the child, bconv_kernel only once (the route call's two
    60-bit limbs) and keypair_dot2_kernel only once (their products)"""
    launched = children.traced(MODEL_PY, [], 600)
    want = rs.kernel_names("modup_mul2_kernel", rs.fused_launch_cases())
    assert len(want) == 36
    assert not sorted(want - set(launched)), "instances never launched: %s" % sorted(want - set(launched))
    assert launched.count("modup_mul2_kernel<ArithF64,14,1>") == 1, launched
    assert not [k for k in launched if k.startswith("modup_mul_kernel<")], launched
    assert not [i.key for i in map(kernel_inventory.parse, launched) if i.family == "fwd_mul_kernel"], launched
    assert launched.count("bconv_kernel") == 1, launched
    assert launched.count("keypair_dot2_kernel") == 1, launched
