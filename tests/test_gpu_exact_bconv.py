"""GPU: the exact base conversion and the exact scaled ModDown (ntt_rns_mod_up_exact_batch, ntt_rns_mod_down_exact_batch and their strided
forms).  Every output word against the model of tests/exact_bconv_model.py: every moddown_exact_fwd_kernel instance with 1, 2 and 4 P
primes, fused == sandwich, the sandwich at 2^15 and 2^16, integer-policy limbs, Q counts across the 16-limb run boundary, exact ModUp in
both domains, the band words (B -+ 1) / 2 planted in the inputs, layouts with canaries, argument errors that write nothing, a BFV
multiplication on real encryptions through the library calls, the plain-C example, and one call captured into a HIP graph."""
import random
import re

import numpy as np
import pytest

import children
import exact_bconv_model as xm
import keyswitch_model as km
import rns_support as rs

T = xm.TRANSFORMED
M = 65537


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [1, 2, 4])
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn, np_):
    """each moddown_exact_fwd_kernel<policy, LOGN, class>: three Q limbs of the class, np 60-bit P limbs, NTT domain, batch 3, m = 65537"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    primes, roots = rs.chain(lib, n, [b] * 3 + [60] * np_)
    xm.run_down(lib, oracle, primes, roots, np_, n, 3, M, T, fused=1, seed=logn + np_)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nq,np_", [(14, 16, 2), (9, 5, 1), (12, 20, 3), (13, 8, 8)])
def test_fused_equals_sandwich_bit_for_bit(lib, oracle, logn, nq, np_):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * np_)
    fused = xm.run_down(lib, oracle, primes, roots, np_, n, 2, M, T, fused=1, seed=3)
    sandwich = xm.run_down(lib, oracle, primes, roots, np_, n, 2, M, T, fused=0, seed=3)
    for a, b in zip(fused, sandwich):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16])
def test_sandwich_at_large_sizes(lib, oracle, logn):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 50, 60, 60])
    xm.run_down(lib, oracle, primes, roots, 2, n, 2, M, T, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T])
def test_integer_policy_limbs(lib, oracle, flags):
    """60-bit kept limbs (the wide integer policy): the coefficient kernel, or the sandwich around it; exact ModUp beside it"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, [60] * 5)
    xm.run_down(lib, oracle, primes, roots, 2, n, 3, M, flags, seed=7)
    xm.run_up(lib, oracle, primes, roots, 1, 2, n, 3, flags, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [5, 17, 18, 34])
@pytest.mark.parametrize("flags", [0, T])
def test_mod_down_q_counts_across_the_run_boundary(lib, oracle, nq, flags):
    """several launches per call, band words in the P limbs: one v for all of them (mult = 1 keeps [m t]_P on the planted values)"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50] * nq + [60, 60, 60])
    xm.run_down(lib, oracle, primes, roots, 3, n, 2, 1, flags, seed=nq, band=True)
    xm.run_down(lib, oracle, primes, roots, 3, n, 2, M, flags, seed=nq + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs,first,count", [(6, 0, 2), (6, 2, 2), (6, 4, 2), (5, 2, 1), (20, 2, 16), (17, 0, 1), (9, 5, 4), (9, 0, 5)])
@pytest.mark.parametrize("flags", [0, T])
@pytest.mark.parametrize("logn", [6, 12])
def test_mod_up_exact(lib, oracle, nlimbs, first, count, flags, logn):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 3) + [60, 60])
    xm.run_up(lib, oracle, primes, roots, first, count, n, 2, flags, seed=nlimbs + first)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,bits", [(2, 50), (4, 50), (16, 60)], ids=["2x50", "4x50", "16x60"])
@pytest.mark.parametrize("flags", [0, T])
def test_band_words_planted_in_the_inputs(lib, oracle, nb, bits, flags):
    """(B - 1) / 2 and (B + 1) / 2 in the digit of an exact ModUp to 18 limbs (two launches) and in the P limbs of an exact ModDown
    (coefficients; NTT domain: the fused kernel and the sandwich): the model's choice in every limb"""
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [bits] * nb + [52] * 18)
    xm.run_up(lib, oracle, primes, roots, 0, nb, n, 2, flags, seed=nb, band=True)
    primes, roots = rs.chain(lib, n, [52] * 18 + [bits] * nb)
    for fused in ((1, 0) if flags & T else (None,)):
        xm.run_down(lib, oracle, primes, roots, nb, n, 2, 1, flags, fused=fused, seed=nb, band=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "limb_padded", "batch_padded"])
@pytest.mark.parametrize("batch", [1, 3, 130])
def test_layouts(lib, oracle, layout, batch):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    for flags in (0, T):
        xm.run_down(lib, oracle, primes, roots, 2, n, batch, M, flags, layout=layout, seed=11)
        xm.run_up(lib, oracle, primes, roots, 1, 2, n, batch, flags, layout=layout, seed=12)


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
    F, A = 2, 4
    down = [
        ("mult 0", p4, 2, 0, T, None, buf.ptr),
        ("mult 2^61", p4, 2, 1 << 61, T, None, buf.ptr),
        ("FLOOR", p4, 2, M, T | F, None, buf.ptr),
        ("ACCUMULATE", p4, 2, M, T | A, None, buf.ptr),
        ("unknown flag", p4, 2, M, 8, None, buf.ptr),
        ("no Q limb", plans[:2], 2, M, T, None, buf.ptr),
        ("no P limb", plans[:2], 0, M, T, None, buf.ptr),
        ("17 P limbs", plans[:18], 17, M, 0, None, buf.ptr),
        ("differing N", [plans[0], other, plans[2], plans[3]], 2, M, T, None, buf.ptr),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 2, M, 0, None, buf.ptr),
        ("overlapping strides", p4, 2, M, T, (n, n), buf.ptr),
        ("null pointer", p4, 2, M, T, None, None),
        ("P limb without its inverse table", [plans[0], plans[1], plans[2], fwd_only], 2, M, T, None, buf.ptr),
    ]
    for what, ps, np_, mult, flags, lay, ptr in down:
        with pytest.raises(lib.NttError):
            lib.rns_mod_down_exact(ps, np_, ptr, mult, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    up = [
        ("count 0", p4, 0, 0, 0, None, buf.ptr),
        ("count 17", plans[:18], 0, 17, 0, None, buf.ptr),
        ("digit past the end", p4, 3, 2, 0, None, buf.ptr),
        ("negative first", p4, -1, 2, 0, None, buf.ptr),
        ("differing N", [plans[0], other, plans[2], plans[3]], 0, 1, 0, None, buf.ptr),
        ("a prime twice", [plans[0], plans[1], plans[2], same], 0, 1, 0, None, buf.ptr),
        ("overlapping strides", p4, 0, 1, T, (n, n), buf.ptr),
        ("unknown flag", p4, 0, 1, 2, None, buf.ptr),
        ("null pointer", p4, 0, 1, 0, None, None),
        ("digit limb without its inverse table", [plans[0], plans[1], plans[2], fwd_only], 3, 1, T, None, buf.ptr),
    ]
    for what, ps, first, count, flags, lay, ptr in up:
        with pytest.raises(lib.NttError):
            lib.rns_mod_up_exact(ps, ptr, first, count, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    # a Q limb without the inverse table: refused where the sandwich serves it, served by the fused route
    fwd_only_q = rs.forward_only_plan(lib, n, primes[1], roots[1])
    ps = [plans[0], fwd_only_q, plans[2], plans[3]]
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 0)
    with pytest.raises(lib.NttError):
        lib.rns_mod_down_exact(ps, 2, buf.ptr, M, batch, T)
    assert np.array_equal(buf.download(), img), "sandwich without an inverse table"
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 1)
    xm.run_down(lib, oracle, primes[:4], roots[:4], 2, n, batch, M, T, plans=ps, seed=9)
    for p in plans + [other, same, fwd_only, fwd_only_q]:
        p.destroy()
    buf.free()


# ---------------------------------------------------------------- BFV through the library calls

@pytest.mark.gpu
@pytest.mark.parametrize("logn", [6, 10])
def test_bfv_multiplication_through_the_library_calls(lib, oracle, logn):
    """real encryptions under a ternary key, Q = 2 x 50 bits, R = 3 x 50 bits, t = 65537: the sequence of examples/rns_bfv_mul.c
    decrypts to m1 m2 mod t, and every word of the result (R limbs included) equals the model"""
    n, nr, nq, t = 1 << logn, 3, 2, 65537
    primes, roots = rs.chain(lib, n, [50] * (nr + nq))
    qp, qr = primes[nr:], roots[nr:]
    Q = km.prod(qp)
    rng = random.Random(logn)
    s = xm.bfv_keygen(rng, n)
    m1, m2 = ([rng.randrange(t) for _ in range(n)] for _ in range(2))
    ct = [p for m in (m1, m2) for p in xm.bfv_encrypt(rng, s, m, n, Q, t)]
    ntt = [[oracle.ctx(n, q, w).fwd(c) for q, w, c in zip(qp, qr, km.residues(p, qp))] for p in ct]
    got = xm.bfv_on_device(lib, primes, roots, nr, t, ntt, n)
    want, (_, _, _, back) = xm.bfv_mul(oracle, primes, roots, nr, t, *ntt, n)
    for j in range(3):
        for l in range(nr + nq):
            assert np.array_equal(got[j][l], back[j][l]), "d%d, limb %d" % (j, l)
    di = [km.crt([oracle.ctx(n, q, w).inv(c) for q, w, c in zip(qp, qr, dj[nr:])], qp) for dj in got]
    assert xm.bfv_decrypt(s, di, n, Q, t) == xm.negacyclic(m1, m2, n, t)


@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_bfv_mul")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r"comp (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    want = xm.example_model(lib, oracle)
    assert len(got) == 12 and got == want, sorted(k for k in want if got.get(k) != want[k])


@pytest.mark.gpu
def test_mod_down_exact_captured_in_a_hip_graph():
    """one ntt_rns_mod_down_exact_batch call (NTT domain, 2^12, four 50-bit Q limbs and two 60-bit P limbs) captured into a HIP graph
    after ntt_plan_reserve and replayed twice on fresh inputs (a process of its own: torch has to be imported before the library)"""
    code = """
import torch
torch.cuda.set_device(0)
import numpy as np
import ontt
from oracle_binding import Oracle
import exact_bconv_model as xm
import rns_support as rs
lib, orc = ontt.load(), Oracle()
n, batch, np_, mult = 1 << 12, 3, 2, 65537
primes, roots = rs.chain(lib, n, [50] * 4 + [60] * np_)
plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
words = len(primes) * batch * n
buf = torch.zeros(words, dtype=torch.int64, device="cuda:0")
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=0)
for p in plans:
    p.reserve(batch * len(primes), stream=s.cuda_stream)
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.graph(g, stream=s):
    st = torch.cuda.current_stream().cuda_stream
    lib.rns_mod_down_exact(plans, np_, buf.data_ptr(), mult, batch, xm.TRANSFORMED, stream=st)
for seed in (1, 2):
    limbs = xm._operand(orc, primes, roots, n, batch, xm.TRANSFORMED, seed)
    buf.copy_(torch.from_numpy(np.concatenate(limbs).view(np.int64)))
    g.replay()
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64).reshape(len(primes), batch * n)
    want, t = xm.mod_down_exact(orc, primes, roots, np_, limbs, n, mult, xm.TRANSFORMED)
    for l, w in enumerate(want + t):
        assert np.array_equal(got[l], w), (seed, l)
print("graph ok")
"""
    children.python_child(code, 300)
