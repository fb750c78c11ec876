"""GPU: the BGV ModDown (ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch and their strided forms).  Every output word against
the model of tests/bgv_model.py: every moddown_bgv_fwd_kernel instance with 1, 2 and 4 P primes in both forms, fused == sandwich, T = 1
against the approximate calls, the sandwich at 2^15 and 2^16, integer-policy limbs, Q counts across the 16-limb run boundary, the edge
words planted in the inputs for every edge T, layouts with canaries, argument errors that write nothing, a BGV multiplication on real
encryptions through the library calls, the plain-C example, and one call of each form captured into a HIP graph."""
import random
import re

import numpy as np
import pytest

import bgv_model as bm
import children
import ct_mul_model as cm
import keyswitch_model as km
import rns_support as rs

T, A = bm.TRANSFORMED, bm.ACCUMULATE
PT = bm.PT


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [1, 2, 4])
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn, np_):
    """each moddown_bgv_fwd_kernel<policy, LOGN, class>: three Q limbs of the class, np 60-bit P limbs, NTT domain, batch 3, T = 65537,
    the in-place form; at np = 2 the add form with ACCUMULATE as well"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    primes, roots = rs.chain(lib, n, [b] * 3 + [60] * np_)
    bm.run_down(lib, oracle, primes, roots, np_, n, 3, PT, T, fused=1, seed=logn + np_)
    if np_ == 2:
        bm.run_down_add(lib, oracle, primes, roots, np_, n, 3, PT, T | A, fused=1, seed=logn, a_untouched=True)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nq,np_", [(14, 16, 2), (9, 5, 1), (12, 20, 3), (13, 8, 8)])
def test_fused_equals_sandwich_bit_for_bit(lib, oracle, logn, nq, np_):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * np_)
    fused = bm.run_down(lib, oracle, primes, roots, np_, n, 2, PT, T, fused=1, seed=3)
    sandwich = bm.run_down(lib, oracle, primes, roots, np_, n, 2, PT, T, fused=0, seed=3)
    for a, b in zip(fused, sandwich):
        assert np.array_equal(a, b)
    fused = bm.run_down_add(lib, oracle, primes, roots, np_, n, 2, PT, T | A, fused=1, seed=4, a_untouched=True)
    sandwich = bm.run_down_add(lib, oracle, primes, roots, np_, n, 2, PT, T | A, fused=0, seed=4)
    for a, b in zip(fused, sandwich):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T])
def test_t_1_equals_the_approximate_calls_bit_for_bit(lib, oracle, flags):
    n, np_ = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50] * 5 + [60] * np_)
    for fused in ((1, 0) if flags & T else (None,)):
        got = bm.run_down(lib, oracle, primes, roots, np_, n, 2, 1, flags, fused=fused, seed=6)
        want = km.run_down(lib, oracle, primes, roots, np_, n, 2, flags, seed=6)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        for acc in (0, A):
            got = bm.run_down_add(lib, oracle, primes, roots, np_, n, 2, 1, flags | acc, fused=fused, seed=7)
            want = cm.run_down_add(lib, oracle, primes, roots, np_, n, 2, flags | acc, seed=7, cross_check=False)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16])
def test_sandwich_at_large_sizes(lib, oracle, logn):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60, 60])
    bm.run_down(lib, oracle, primes, roots, 2, n, 2, PT, T, seed=logn)
    bm.run_down_add(lib, oracle, primes, roots, 2, n, 2, PT, T | A, seed=logn + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T])
def test_integer_policy_limbs(lib, oracle, flags):
    """60-bit kept limbs (the wide integer policy): the coefficient kernel, or the sandwich around it"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, [60] * 5)
    bm.run_down(lib, oracle, primes, roots, 2, n, 3, PT, flags, seed=7)
    bm.run_down_add(lib, oracle, primes, roots, 2, n, 3, PT, flags | A, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [5, 17, 18, 34])
@pytest.mark.parametrize("flags", [0, T])
def test_q_counts_across_the_run_boundary(lib, oracle, nq, flags):
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * nq + [60, 60, 60])
    bm.run_down(lib, oracle, primes, roots, 3, n, 2, PT, flags, seed=nq)
    bm.run_down_add(lib, oracle, primes, roots, 3, n, 2, PT, flags | A, seed=nq + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [1, 2, 16])
@pytest.mark.parametrize("ti", range(5), ids=["T1", "T2", "T65537", "T61bit", "Tq0"])
def test_edge_words_planted_in_the_inputs(lib, oracle, np_, ti):
    """t_j in {0, 1, (p - 1) / 2, (p + 1) / 2, p - 1} with c in {0, q - 1} in front of every polynomial, for every edge T (T = q_0 makes
    [T]_{q_0} = 0): coefficients, the fused kernel and the sandwich, the add form beside the in-place one"""
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50, 52, 51] + [60] * np_)
    pt = bm.edge_ts(primes)[ti]
    bm.run_down(lib, oracle, primes, roots, np_, n, 2, pt, 0, seed=ti, edges=True)
    for fused in (1, 0):
        bm.run_down(lib, oracle, primes, roots, np_, n, 2, pt, T, fused=fused, seed=ti, edges=True)
    bm.run_down_add(lib, oracle, primes, roots, np_, n, 2, pt, T | A, fused=1, seed=ti, edges=True, a_untouched=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "limb_padded", "batch_padded"])
@pytest.mark.parametrize("batch", [1, 3, 130])
def test_layouts(lib, oracle, layout, batch):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    other = {"limb": "batch_padded", "batch": "limb_padded", "limb_padded": "batch", "batch_padded": "limb"}[layout]
    for flags in (0, T):
        bm.run_down(lib, oracle, primes, roots, 2, n, batch, PT, flags, layout=layout, seed=11)
        bm.run_down_add(lib, oracle, primes, roots, 2, n, batch, PT, flags | A, c_layout=layout, a_layout=other, seed=12,
                        a_untouched=bool(flags & T))
    bm.run_down_add(lib, oracle, primes, roots, 2, n, batch, PT, T, c_layout=layout, a_layout=layout, fused=0, seed=13)


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
    cimg = oracle.fill_uniform(words, primes[0], 6)
    buf, cbuf = lib.DeviceBuffer(words).upload(img), lib.DeviceBuffer(words).upload(cimg)
    p4 = plans[:4]
    F = 2
    cases = [
        ("t 0", p4, 2, 0, T, None),
        ("t 2^61", p4, 2, 1 << 61, T, None),
        ("a P prime divides t", p4, 2, 3 * primes[3], T, None),
        ("t is a P prime", p4, 2, primes[2], 0, None),
        ("FLOOR", p4, 2, PT, T | F, None),
        ("unknown flag", p4, 2, PT, 8, None),
        ("no Q limb", plans[:2], 2, PT, T, None),
        ("no P limb", plans[:2], 0, PT, T, None),
        ("17 P limbs", plans[:18], 17, PT, 0, None),
        ("differing N", [plans[0], other, plans[2], plans[3]], 2, PT, T, None),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 2, PT, 0, None),
        ("overlapping strides", p4, 2, PT, T, (n, n)),
        ("P limb without its inverse table", [plans[0], plans[1], plans[2], fwd_only], 2, PT, T, None),
    ]

    def unchanged(what):
        assert np.array_equal(buf.download(), img) and np.array_equal(cbuf.download(), cimg), what

    for what, ps, np_, pt, flags, lay in cases:
        with pytest.raises(lib.NttError):
            lib.rns_mod_down_bgv(ps, np_, buf.ptr, pt, batch, flags, layout=lay)
        unchanged(what)
        with pytest.raises(lib.NttError):
            lib.rns_mod_down_bgv_add(ps, np_, cbuf.ptr, buf.ptr, pt, batch, flags, layout=(lay + lay) if lay else None)
        unchanged(what + " (add form)")
    for what, call in [
        ("ACCUMULATE in place", lambda: lib.rns_mod_down_bgv(p4, 2, buf.ptr, PT, batch, T | A)),
        ("null operand", lambda: lib.rns_mod_down_bgv(p4, 2, None, PT, batch, T)),
        ("null accumulator", lambda: lib.rns_mod_down_bgv_add(p4, 2, cbuf.ptr, None, PT, batch, T)),
        ("null ciphertext", lambda: lib.rns_mod_down_bgv_add(p4, 2, None, buf.ptr, PT, batch, T)),
        ("d_c overlaps d_a", lambda: lib.rns_mod_down_bgv_add(p4, 2, buf.ptr + 8 * n, buf.ptr, PT, batch, T)),
        ("overlapping ciphertext strides", lambda: lib.rns_mod_down_bgv_add(p4, 2, cbuf.ptr, buf.ptr, PT, batch, T,
                                                                           layout=(n, n, batch * n, n))),
    ]:
        with pytest.raises(lib.NttError):
            call()
        unchanged(what)
    # a Q limb without the inverse table: refused where the sandwich serves it, served by the fused route
    fwd_only_q = rs.forward_only_plan(lib, n, primes[1], roots[1])
    ps = [plans[0], fwd_only_q, plans[2], plans[3]]
    plans[0].set_option(lib.OPT_BGV_FUSED, 0)
    with pytest.raises(lib.NttError):
        lib.rns_mod_down_bgv(ps, 2, buf.ptr, PT, batch, T)
    unchanged("sandwich without an inverse table")
    bm.run_down(lib, oracle, primes[:4], roots[:4], 2, n, batch, PT, T, fused=1, plans=ps, seed=9)
    assert plans[0].get_option(lib.OPT_BGV_FUSED) == -1, "the runner puts the default back"
    for p in plans + [other, same, fwd_only, fwd_only_q]:
        p.destroy()
    buf.free(), cbuf.free()


# ---------------------------------------------------------------- BGV through the library calls

@pytest.mark.gpu
def test_bgv_multiplication_through_the_library_calls(lib, oracle):
    """N = 2^10, Q = 4 x 50 bits, P = 2 x 60 bits, two digits of two limbs, T = 65537, three ciphertext pairs of real encryptions under a
    ternary key: tensor, inverse of d2, the pair key products per digit, the BGV ModDown into (d0, d1), the BGV switch by q_3.  Every
    word equals the model, the relinearised product decrypts to m1 m2 and the switched one to m1 m2 q_3^-1 mod T"""
    n, nq, npp = 1 << 10, 4, 2
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * npp)
    rng = random.Random(10)
    bgv = bm.Bgv(oracle, primes, roots, nq, 2, n, PT, rng)
    keys = bgv.relin_keys()
    f = pow(primes[nq - 1], -1, PT)
    for _ in range(3):
        m1, m2 = ([rng.randrange(PT) for _ in range(n)] for _ in range(2))
        ct1, ct2 = bgv.encrypt(m1), bgv.encrypt(m2)
        relin, switched = bm.mul_on_device(lib, bgv, ct1, ct2, keys)
        want_sw, want_relin, _ = bgv.multiply(ct1, ct2, keys)
        for j in range(2):
            for l in range(nq):
                assert np.array_equal(relin[j][l], want_relin[j][l]), "relinearised d%d, limb %d" % (j, l)
            for l in range(nq - 1):
                assert np.array_equal(switched[j][l], want_sw[j][l]), "switched d%d, limb %d" % (j, l)
        want = bgv.plain_product(m1, m2)
        assert bgv.decrypt(relin, nq) == want
        assert bgv.decrypt(switched, nq - 1) == [v * f % PT for v in want]


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_bgv_mul")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r"comp (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    want = bm.example_model(lib, oracle)
    assert len(got) == 14 and got == want, sorted(k for k in want if got.get(k) != want[k])


@pytest.mark.gpu
def test_both_forms_captured_in_a_hip_graph():
    """one ntt_rns_mod_down_bgv_batch call and one ntt_rns_mod_down_bgv_add_batch call (NTT domain, 2^12, four 50-bit Q limbs and two
    60-bit P limbs) captured one after the other on one stream into a HIP graph after ntt_plan_reserve (a linear capture) and replayed
    twice on fresh inputs (a process of its own: torch has to be imported before the library)"""
    code = """
import torch
torch.cuda.set_device(0)
import numpy as np
import ontt
from oracle_binding import Oracle
import bgv_model as bm
import keyswitch_model as km
import rns_support as rs
lib, orc = ontt.load(), Oracle()
n, batch, np_, pt = 1 << 12, 3, 2, 65537
T, A = bm.TRANSFORMED, bm.ACCUMULATE
primes, roots = rs.chain(lib, n, [50] * 4 + [60] * np_)
nq = len(primes) - np_
plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
words = len(primes) * batch * n
buf = torch.zeros(words, dtype=torch.int64, device="cuda:0")
acc = torch.zeros(words, dtype=torch.int64, device="cuda:0")
ct = torch.zeros(nq * batch * n, dtype=torch.int64, device="cuda:0")
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=0)
for p in plans:
    p.reserve(batch * len(primes), stream=s.cuda_stream)
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.graph(g, stream=s):
    st = torch.cuda.current_stream().cuda_stream
    lib.rns_mod_down_bgv(plans, np_, buf.data_ptr(), pt, batch, T, stream=st)
    lib.rns_mod_down_bgv_add(plans, np_, ct.data_ptr(), acc.data_ptr(), pt, batch, T | A, stream=st)
for seed in (1, 2):
    limbs = km._operand(orc, primes, roots, n, batch, T, seed)
    a = km._operand(orc, primes, roots, n, batch, T, seed + 10)
    c = km._operand(orc, primes[:nq], roots[:nq], n, batch, T, seed + 20)
    buf.copy_(torch.from_numpy(np.concatenate(limbs).view(np.int64)))
    acc.copy_(torch.from_numpy(np.concatenate(a).view(np.int64)))
    ct.copy_(torch.from_numpy(np.concatenate(c).view(np.int64)))
    g.replay()
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64).reshape(len(primes), batch * n)
    want, t = bm.mod_down_bgv(orc, primes, roots, np_, limbs, n, pt, T)
    for l, w in enumerate(want + t):
        assert np.array_equal(got[l], w), ("in place", seed, l)
    got = ct.cpu().numpy().view(np.uint64).reshape(nq, batch * n)
    want, t = bm.mod_down_bgv_add(orc, primes, roots, np_, c, a, n, pt, T | A)
    for l, w in enumerate(want):
        assert np.array_equal(got[l], w), ("add", seed, l)
print("graph ok")
"""
    children.python_child(code, 300)
