"""CPU: the exact base conversion and the exact scaled ModDown (ntt_rns_mod_up_exact_batch, ntt_rns_mod_down_exact_batch) without a GPU
-- the model of tests/exact_bconv_model.py against the definitions with Python integers (the centred x; round(m x / P)) on values
chosen outside the band |2x - B| <= 2^-43 B, the band values themselves, the relation to the approximate ModDown, a toy BFV
multiplication that decrypts, the host side of csrc/ntt_exact.h bit for bit against the model (tests/exact_host_check.cpp), the
exported symbols, the plain-C example against the public header alone and the kernels of the new translation unit."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import children
import exact_bconv_model as xm
import keyswitch_model as km
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")
LIB = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
T = xm.TRANSFORMED
N = 64
MULTS = [1, 65537, (1 << 59) + 12345]


# (source bits, destination bits) and the reverse directions
_FWD = [([30], [30, 30]), ([50] * 2, [60] * 3), ([50] * 4, [50] * 5), ([60] * 8, [60] * 9), ([60] * 16, [52] * 16)]
CHAINS = _FWD + [(d, s) for s, d in _FWD]
CHAIN_IDS = ["%dx%d-%dx%d" % (len(s), s[0], len(d), d[0]) for s, d in CHAINS]


def _split(orc, src_bits, dst_bits):
    """(source primes, roots), (destination primes, roots): distinct primes even where the bit sizes coincide"""
    primes, roots = rs.chain(orc, N, src_bits + dst_bits)
    ns = len(src_bits)
    return (primes[:ns], roots[:ns]), (primes[ns:], roots[ns:])


def _chosen(limit, B, fixed, count, rng, image=lambda x: x):
    """the fixed values, then random ones below limit, every one with image(x) outside the band of B: the fixed ones are asserted to
    be, a random one inside is drawn again (none is dropped)"""
    xs = list(fixed)
    for x in xs:
        assert xm.outside_band(image(x), B), x
    while len(xs) < count:
        x = rng.randrange(limit)
        if xm.outside_band(image(x), B):
            xs.append(x)
    return xs


@pytest.mark.parametrize("src_bits,dst_bits", CHAINS, ids=CHAIN_IDS)
@pytest.mark.parametrize("flags", [0, T])
def test_mod_up_exact_model_gives_the_centred_value(oracle, src_bits, dst_bits, flags):
    (sp, sr), (dp, dr) = _split(oracle, src_bits, dst_bits)
    primes, roots, count = sp + dp, sr + dr, len(sp)
    B = km.prod(sp)
    rng = random.Random(len(src_bits) * 100 + len(dst_bits) + flags)
    xs = _chosen(B, B, [0, 1, B - 1], N, rng)
    coef = km.residues(xs, sp) + [oracle.fill_uniform(N, q, 50 + l) for l, q in enumerate(dp)]
    limbs = [oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    got = xm.mod_up_exact(oracle, primes, roots, limbs, N, 0, count, flags)
    for l, (q, w) in enumerate(zip(primes, roots)):
        if l < count:
            assert np.array_equal(got[l], limbs[l]), "the digit's limb %d changed" % l
            continue
        c = oracle.ctx(N, q, w).inv(got[l]) if flags & T else got[l]
        assert c.tolist() == [xm.centred(x, B) % q for x in xs], "limb %d" % l
        # the Python-integer form of the model: the same words
        want, _ = xm.exact_bconv_int(sp, coef[:count], q)
        assert c.tolist() == want


@pytest.mark.parametrize("src_bits,dst_bits", CHAINS, ids=CHAIN_IDS)
@pytest.mark.parametrize("mult", MULTS, ids=["m1", "m65537", "m60bit"])
@pytest.mark.parametrize("flags", [0, T])
def test_mod_down_exact_model_gives_the_rounded_quotient(oracle, src_bits, dst_bits, mult, flags):
    """P = the source basis, Q = the destination basis: round(m x / P) mod q_l for x in [0, QP), [m x]_P outside the band"""
    (pp, prr), (qp, qr) = _split(oracle, src_bits, dst_bits)
    primes, roots, nq, np_ = qp + pp, qr + prr, len(qp), len(pp)
    Q, P = km.prod(qp), km.prod(pp)
    rng = random.Random(len(src_bits) * 100 + len(dst_bits) + flags + mult % 1000)
    xs = _chosen(Q * P, P, [0, 1, Q * P - 1], N, rng, lambda x: mult * x % P)
    coef = km.residues(xs, primes)
    limbs = [oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & T else coef
    got, t = xm.mod_down_exact(oracle, primes, roots, np_, limbs, N, mult, flags)
    for j in range(np_):
        assert np.array_equal(t[j], coef[nq + j]), "t is the P limbs' coefficients"
    for l, (q, w) in enumerate(zip(qp, qr)):
        c = oracle.ctx(N, q, w).inv(got[l]) if flags & T else got[l]
        assert c.tolist() == [(2 * mult * x + P) // (2 * P) % q for x in xs], "limb %d" % l


@pytest.mark.parametrize("nb,bits", [(2, 50), (4, 50), (16, 60), (1, 30)], ids=["2x50", "4x50", "16x60", "1x30"])
def test_band_values_take_one_choice_in_every_limb(oracle, nb, bits):
    """(B - 1) / 2, (B + 1) / 2 and (B - 1) / 2 +- 2^10: every limb holds x - v' B for ONE v' in {0, 1}; the exact ModDown of a value
    whose remainder is one of them is the floor or the ceiling in every limb"""
    (sp, _), (dp, _) = _split(oracle, [bits] * nb, [52] * 5)
    B = km.prod(sp)
    xs = [(B - 1) // 2, (B + 1) // 2, (B - 1) // 2 + 1024, (B - 1) // 2 - 1024]
    got = [xm.exact_bconv(oracle, sp, km.residues(xs, sp), q)[0] for q in dp]
    for i, x in enumerate(xs):
        picks = {vp for vp in (0, 1) if all(int(g[i]) == (x - vp * B) % q for g, q in zip(got, dp))}
        assert picks, "x = %d: the limbs do not agree on x or x - B" % x
    # ModDown over Q = dp, P = sp: x = k P + r with r a band value
    rng = random.Random(nb)
    Q = km.prod(dp)
    for mult in (1, 65537):
        ys = [((rng.randrange(Q) * B + r) * pow(mult, -1, Q * B)) % (Q * B) for r in xs]
        assert [mult * y % B for y in ys] == [r % B for r in xs]
        out, _ = xm.mod_down_exact(oracle, dp + sp, [0] * (len(dp) + nb), nb, km.residues(ys, dp + sp), len(ys), mult, 0)
        for i, y in enumerate(ys):
            lo = mult * y // B
            picks = {e for e in (0, 1) if all(int(o[i]) == (lo + e) % q for o, q in zip(out, dp))}
            assert picks, "y = %d: neither the floor nor the ceiling in every limb" % y


@pytest.mark.parametrize("qbits,pbits", [([50] * 16, [60, 60]), ([50] * 4, [50, 50, 50]), ([60] * 5, [60] * 8), ([50, 50], [60])],
                         ids=["q16x50-p2x60", "q4x50-p3x50", "q5x60-p8x60", "q2x50-p1x60"])
def test_exact_mod_down_is_the_approximate_one_plus_its_error(oracle, qbits, pbits):
    """mult = 1: exact = round(x / P), the existing call's round(x / P) - v with 0 <= v < np: the difference is that v in every limb,
    and the words are equal where v = 0"""
    primes, roots = rs.chain(oracle, N, qbits + pbits)
    nq, np_ = len(qbits), len(pbits)
    P = km.prod(primes[nq:])
    coef = [oracle.fill_uniform(N, q, 70 + l) for l, q in enumerate(primes)]
    exact, _ = xm.mod_down_exact(oracle, primes, roots, np_, coef, N, 1, 0)
    approx, _ = km.mod_down(oracle, primes, roots, np_, coef, N, 0)
    h = (P - 1) // 2
    sums = km.fastbconv_int(primes[nq:], coef[nq:], [h % p for p in primes[nq:]])
    r = [(x + h) % P for x in km.crt(coef[nq:], primes[nq:])]
    vs = [(s - ri) // P for s, ri in zip(sums, r)]
    assert all(0 <= v < np_ for v in vs)
    if np_ > 1:
        assert any(vs), "the case exercises no error"
    for l, q in enumerate(primes[:nq]):
        assert [(int(a) + v) % q for a, v in zip(approx[l], vs)] == exact[l].tolist(), "limb %d" % l
        same = np.array([v == 0 for v in vs])
        assert np.array_equal(exact[l][same], approx[l][same])


def test_toy_bfv_multiplication_decrypts(oracle):
    """N = 64, Q = 2 x 50 bits, R = 3 x 50 bits, t = 65537, real encryptions under a ternary key: the five-call sequence on the model
    decrypts to m1 m2 mod t"""
    nr, nq, t = 3, 2, 65537
    primes, roots = rs.chain(oracle, N, [50] * (nr + nq))
    qp, qr = primes[nr:], roots[nr:]
    Q = km.prod(qp)
    rng = random.Random(2024)
    s = xm.bfv_keygen(rng, N)
    m1, m2 = ([rng.randrange(t) for _ in range(N)] for _ in range(2))
    ct = [p for m in (m1, m2) for p in xm.bfv_encrypt(rng, s, m, N, Q, t)]  # a0, a1, b0, b1 as integers mod Q
    assert xm.bfv_decrypt(s, ct[:2], N, Q, t) == m1 and xm.bfv_decrypt(s, ct[2:], N, Q, t) == m2
    ntt = [[oracle.ctx(N, q, w).fwd(c) for q, w, c in zip(qp, qr, km.residues(p, qp))] for p in ct]
    d, _ = xm.bfv_mul(oracle, primes, roots, nr, t, *ntt, N)
    di = [km.crt([oracle.ctx(N, q, w).inv(c) for q, w, c in zip(qp, qr, dj)], qp) for dj in d]
    assert xm.bfv_decrypt(s, di, N, Q, t) == xm.negacyclic(m1, m2, N, t)


# ---------------------------------------------------------------- the host side of csrc/ntt_exact.h

@pytest.fixture(scope="module")
def host_check():
    return children.build_host_check("exact_host_check", "-O2 -std=c++17 -ffp-contract=off")


def _host(exe, tmp_path, mode, basis, dest, mult, rows):
    path = os.path.join(str(tmp_path), "vec.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n%s\n" % (mode, len(basis), len(dest), mult, len(rows), " ".join(map(str, basis)), " ".join(map(str, dest))))
        for row in rows:
            f.write(" ".join(str(int(v)) for v in row) + "\n")
    out = subprocess.check_output([exe, path], text=True)
    return [[int(v) for v in line.split()] for line in out.splitlines()]


@pytest.mark.parametrize("src_bits,dst_bits", [([30], [30, 30]), ([50] * 2, [60] * 3), ([50] * 4, [50] * 5), ([60] * 16, [52] * 16), ([52] * 16, [60] * 16)],
                         ids=["1x30", "2x50", "4x50", "16x60", "16x52"])
def test_host_functions_equal_the_model_bit_for_bit(oracle, host_check, tmp_path, src_bits, dst_bits):
    """exact_bconv and moddown_exact_word of csrc/ntt_exact.h, compiled for the host, on random words and on the band values: the
    model's words, the choice inside the band included"""
    (sp, _), (dp, _) = _split(oracle, src_bits, dst_bits)
    B = km.prod(sp)
    band = km.residues([(B - 1) // 2, (B + 1) // 2, (B - 1) // 2 + 1024, (B - 1) // 2 - 1024, 0, 1, B - 1], sp)
    words = [np.concatenate([b, oracle.fill_uniform(N, p, 90 + i)]) for i, (p, b) in enumerate(zip(sp, band))]
    k = len(words[0])
    got = _host(host_check, tmp_path, 0, sp, dp, 1, [[w[i] for w in words] for i in range(k)])
    for d, q in enumerate(dp):
        want, _ = xm.exact_bconv(oracle, sp, words, q)
        assert [row[d] for row in got] == want.tolist(), "conversion to limb %d" % d
    for mult in MULTS:
        c = [oracle.fill_uniform(k, q, 300 + d) for d, q in enumerate(dp)]
        got = _host(host_check, tmp_path, 1, sp, dp, mult, [[w[i] for w in words] + [x[i] for x in c] for i in range(k)])
        want, _ = xm.mod_down_exact(oracle, dp + sp, [0] * (len(dp) + len(sp)), len(sp), c + words, k, mult, 0)
        for d in range(len(dp)):
            assert [row[d] for row in got] == want[d].tolist(), "ModDown, mult %d, limb %d" % (mult, d)


# ---------------------------------------------------------------- build checks

SYMBOLS = {"ntt_rns_mod_up_exact_batch", "ntt_rns_mod_up_exact_batch_strided", "ntt_rns_mod_down_exact_batch",
           "ntt_rns_mod_down_exact_batch_strided"}


def test_exports_the_four_symbols_and_binds_them(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOLS <= names
    assert SYMBOLS <= set(lib.EXPORTED_SYMBOLS)
    assert callable(lib.rns_mod_up_exact) and callable(lib.rns_mod_down_exact)


def test_bfv_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_bfv_mul", *children.STRICT))


def test_exact_objects_hold_exactly_the_expected_instances_without_spills():
    """ksexact_f64*.o and exact_coef.o: one moddown_exact_fwd_kernel per (policy, class, LOGN) of the launch cases and the two coefficient
    kernels, none spilling vector registers or using scratch (where the objects are not at hand: the same kernels of the linked library)"""
    import glob

    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "ksexact_*.o")) + glob.glob(os.path.join(CSRC, "exact_coef.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if "exact_" in k["name"]]
    names = [k["name"] for k in ks]
    by = {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}
    want = rs.kernel_names("moddown_exact_fwd_kernel", rs.fused_launch_cases())
    want |= {"exact_up_coef_kernel", "exact_down_coef_kernel"}
    assert len(want) == 38
    assert set(by) == want, ("missing %s, unexpected %s" % (sorted(want - set(by))[:8], sorted(set(by) - want)[:8]))
    bad = {n: (k.get("vgpr_spill_count"), k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size")) for n, k in by.items()
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0) or k.get("group_segment_fixed_size", 0) > 160 * 1024}
    assert not bad, "spills / scratch / LDS: %s" % bad
