"""Model of the lifts into the RNS (ntt_rns_from_plain_batch, ntt_rns_from_double_batch) for the tests: the three definitions of
include/ntt_mi355x.h in Python big integers, generators of corner words, and the GPU case runner.  Every definition fixes every output
word: the comparisons are bit for bit, there is no band and no tolerance.

Script mode (`python3 tests/lift_model.py`, a fresh process under a kernel trace): one call per lift kernel instance -- every
lift_fwd_kernel (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W) and lift_coef_kernel -- each checked against the model (the
launch proof); `--route`: one NTT-domain call at 2^14 over 17 FP64 limbs (the route proof).
"""
import sys
from math import prod

import numpy as np

import rns_support as rs

SCALE, TRANSFORMED, ACCUMULATE = 1, 2, 4
CENTRED, SCALED, DOUBLE = "centred", "scaled", "double"
TS = [2, 3, 256, 65537, 1 << 32, 1 << 60, (1 << 61) - 1, 10 ** 18 + 9]


# ---------------------------------------------------------------- the definitions (Python integers)

def centred(m, t):
    """m_c = m if 2m < t else m - t: in [-ceil(t/2), t/2)"""
    return m if 2 * m < t else m - t


def scaled(m, t, Q):
    """floor((Q m + floor(t/2)) / t)"""
    return (Q * m + t // 2) // t


def rounded(ybits, scale):
    """v = rint(fl(y * scale)), ties to even; 0 for NaN, inf and |p| >= 2^127"""
    y = np.array([ybits], dtype=np.uint64).view(np.float64)
    with np.errstate(all="ignore"):
        p = y * np.float64(scale)
    if not np.isfinite(p[0]) or abs(p[0]) >= 2.0 ** 127:
        return 0
    return int(np.rint(p)[0])


def integers(mode, plain, primes, t=0, scale=1.0):
    """the integer behind every plaintext word (a list of Python ints); plain: uint64 words, or bit patterns of doubles"""
    words = [int(w) for w in np.asarray(plain, dtype=np.uint64)]
    if mode == CENTRED:
        return [centred(m, t) for m in words]
    if mode == SCALED:
        Q = prod(primes)
        return [scaled(m, t, Q) for m in words]
    with np.errstate(all="ignore"):  # rounded(), on the whole array
        p = np.asarray(plain, dtype=np.uint64).view(np.float64) * np.float64(scale)
        keep = np.isfinite(p) & (np.abs(p) < 2.0 ** 127)
        v = np.rint(np.where(keep, p, 0.0))
    return [int(x) for x in v]


def lift(mode, plain, primes, t=0, scale=1.0):
    """[limb] arrays of canonical words: the definition"""
    vs = integers(mode, plain, primes, t, scale)
    return [np.array([v % q for v in vs], dtype=np.uint64) for q in primes]


def mode_of(kind, flags):
    return DOUBLE if kind == DOUBLE else (SCALED if flags & SCALE else CENTRED)


# ---------------------------------------------------------------- corner words

def plain_corners(t, primes=None):
    """m in {0, 1, ceil(t/2) - 1, ceil(t/2), t - 1}; with primes (the scaled mode): r m + floor(t/2) just below and at a multiple of t,
    and for even t the ties r m = t/2 (mod t) where they exist"""
    up = t - t // 2
    ms = [0, 1 % t, (up - 1) % t, up % t, t - 1]
    if primes:
        from math import gcd
        r = prod(primes) % t
        g = gcd(r, t)
        if r:
            # r m = k (mod t) is solvable iff g | k; the targets: -floor(t/2) (the sum is a multiple of t), one below it, and t/2 (a tie)
            inv = pow(r // g, -1, t // g) if t // g > 1 else 0
            for target in (-(t // 2), -(t // 2) - 1, t // 2, t // 2 - 1):
                k = target % t
                k -= k % g  # the nearest solvable residue at or below the target
                ms.append((k // g) * inv % (t // g))
    return sorted(set(ms))


def double_corners():
    """bit patterns: +-0.0, +-0.5, 1.5, 2.5, 2^53 + 1 (not a double: 2^53 + 2), just below 2^127, 2^127, NaN, +-inf, the smallest
    subnormal, and values whose product with a scale of 1/3 or 3 rounds"""
    vals = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -1.5, -2.5, 2.0 ** 53 + 2, 2.0 ** 53, -(2.0 ** 53) - 2, float(np.nextafter(2.0 ** 127, 0)),
            -float(np.nextafter(2.0 ** 127, 0)), 2.0 ** 127, -(2.0 ** 127), float("nan"), float("inf"), float("-inf"), 5e-324, -5e-324,
            1.0 / 3.0, 7.0, 1e18, -1e30, 2.0 ** 64, 2.0 ** 100 + 2.0 ** 60, 3.5, 4.5, 2.0 ** 126, float(np.nextafter(2.0 ** 64, 0))]
    return np.array(vals, dtype=np.float64).view(np.uint64)


def random_plain(kind, count, t, seed):
    rng = np.random.default_rng(seed)
    if kind == DOUBLE:
        mant = rng.standard_normal(count)
        expo = rng.integers(-4, 70, size=count)
        return (mant * np.exp2(expo)).astype(np.float64).view(np.uint64)
    return rng.integers(0, t, size=count, dtype=np.uint64)


def with_corners(kind, count, t, seed, flags, primes):
    """`count` random words with the corner words at the front (as many as fit)"""
    m = random_plain(kind, count, t, seed)
    c = double_corners() if kind == DOUBLE else np.array(plain_corners(t, primes if flags & SCALE else None), dtype=np.uint64)
    k = min(c.size, count)
    m[:k] = c[:k]
    return m


# ---------------------------------------------------------------- GPU case runner

CANARY = 0xC0FFEE11F7ED0B5E


def expected(orc, kind, plain, primes, roots, n, flags, t=0, scale=1.0, acc_in=None):
    """the output limbs: the definition, through the oracle's forward transform with TRANSFORMED, added to acc_in with ACCUMULATE"""
    out = lift(mode_of(kind, flags), plain, primes, t, scale)
    if flags & TRANSFORMED:
        out = [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, out)]
    if flags & ACCUMULATE:
        out = [((a.astype(object) + c.astype(object)) % q).astype(np.uint64) for a, c, q in zip(acc_in, out, primes)]
    return out


def check_lift(lib, orc, primes, roots, n, batch, kind, flags, t=65537, scale=1.0, plain=None, layout="limb", m_stride=None, fused=None,
               max_grid=None, arith=None, seed=1, plans=None):
    """one call, checked word for word.  The plaintext ([batch][N] at stride m_stride) and the output (layout: rns_support's kinds)
    sit among canaries (64 words either side and in every gap), which must stay untouched, as the plaintext must.  Without ACCUMULATE
    the output slots start as canaries too: every word must be written.  kind: "plain" or "double".  Returns the output limbs."""
    nl, pad = len(primes), 64
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w, **({"arith": arith} if arith else {})) for q, w in zip(primes, roots)]
    if fused is not None:
        plans[0].set_option(lib.OPT_LIFT_FUSED, fused)
    if max_grid is not None:
        for p in plans:
            p.set_option(lib.OPT_MAX_GRID, max_grid)
    if plain is None:
        plain = with_corners(kind, batch * n, t, seed, flags, primes)
    plain = np.asarray(plain, dtype=np.uint64)
    ms = m_stride or n
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    acc_in = [orc.fill_uniform(batch * n, q, seed * 977 + l) for l, q in enumerate(primes)] if flags & ACCUMULATE else None
    if acc_in is not None and batch * n >= 2:
        for a, q in zip(acc_in, primes):
            a[:2] = [q - 1, 0]
    img_c = rs.place(acc_in, n, batch, ls, ps, words) if acc_in is not None else np.full(words, rs.CANARY, dtype=np.uint64)
    host_c = np.concatenate([np.full(pad, CANARY, dtype=np.uint64), img_c, np.full(pad, CANARY, dtype=np.uint64)])
    host_m = np.full((batch - 1) * ms + n + 2 * pad, CANARY, dtype=np.uint64)
    for p in range(batch):
        host_m[pad + p * ms:pad + p * ms + n] = plain[p * n:(p + 1) * n]
    dc, dm = lib.DeviceBuffer(host_c.size).upload(host_c), lib.DeviceBuffer(host_m.size).upload(host_m)
    lay = None if (layout == "limb" and ms == n) else (ls, ps, ms)
    try:
        if kind == DOUBLE:
            lib.rns_from_double(plans, dc.ptr + 8 * pad, dm.ptr + 8 * pad, scale, batch, flags, layout=lay)
        else:
            lib.rns_from_plain(plans, dc.ptr + 8 * pad, dm.ptr + 8 * pad, t, batch, flags, layout=lay)
        got_c, got_m = dc.download(), dm.download()
    finally:
        dc.free()
        dm.free()
        if fused is not None:
            plans[0].set_option(lib.OPT_LIFT_FUSED, -1)
        if own:
            for p in plans:
                p.destroy()
    assert np.array_equal(got_m, host_m), "the plaintext changed"
    assert np.array_equal(got_c[:pad], host_c[:pad]) and np.array_equal(got_c[-pad:], host_c[-pad:]), "a word around the output changed"
    got, used = rs.extract(got_c[pad:-pad], nl, n, batch, ls, ps)
    assert np.array_equal(got_c[pad:-pad][~used], img_c[~used]), "a word in a gap of the output changed"
    want = expected(orc, kind, plain, primes, roots, n, flags, t, scale, acc_in)
    for l in range(nl):
        bad = np.nonzero(got[l] != want[l])[0]
        assert bad.size == 0, "limb %d of %d (N=%d, batch %d, %s, flags %d, %s): words %s got %s want %s" % (
            l, nl, n, batch, kind, flags, layout, bad[:6].tolist(), got[l][bad[:6]].tolist(), want[l][bad[:6]].tolist())
    return got


def instance_case(logn):
    """(kind, flags, t or scale) for the per-instance cases: mode and accumulation rotate with logn"""
    kind, fl, par = [("plain", 0, 65537), ("plain", SCALE, (1 << 61) - 1), (DOUBLE, 0, 2.0 ** 40)][logn % 3]
    return kind, fl | TRANSFORMED | (ACCUMULATE if (logn // 3) % 2 else 0), par


def run_instance(lib, orc, pol, k, logn, **kw):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [rs.CLASS_BITS[(pol, k)]] * 3)
    kind, flags, par = instance_case(logn)
    arg = {"scale": par} if kind == DOUBLE else {"t": par}
    return check_lift(lib, orc, primes, roots, n, 3 if logn < 9 else 2, kind, flags, seed=logn, fused=1, **arg, **kw)


def route(lib, orc):
    """2^14, 17 limbs of 50-bit primes (two runs of the FP64 policy: 16 + 1), NTT domain, 2 polynomials, the fused kernel selected
    (NTT_OPT_LIFT_FUSED 1: the measured default stores a centred lift at 2^14 through the composition): the route proof's call"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, [50] * 17)
    check_lift(lib, orc, primes, roots, n, 2, "plain", TRANSFORMED, fused=1, seed=17)
    print("lift route: one call at 2^14 over 17 limbs")


def example_model(lib, orc):
    """the lines examples/rns_encrypt.c prints: c0^ = pk0^ (.) u^ + e^ + fwd(the lift) per limb, pk0^ = -(a^ (.) s^)"""
    n, t, L, delta = 1 << 13, 65537, 3, 2.0 ** 30
    primes, roots = rs.chain(lib, n, [50] * L)
    m = orc.fill_uniform(n, t, 1)
    u, e, s = orc.fill_uniform(n, 2, 2), orc.fill_uniform(n, 2, 3), orc.fill_uniform(n, 2, 4)
    y = (orc.fill_uniform(n, 1 << 20, 5).astype(np.float64) - 524288.0) / 1024.0
    lifts = {"bfv": lift(SCALED, m, primes, t), "ckks": lift(DOUBLE, y.view(np.uint64), primes[:2], scale=delta)}
    lines = []
    for what in ("bfv", "ckks"):
        for l, pt in enumerate(lifts[what]):
            q, cx = primes[l], orc.ctx(n, primes[l], roots[l])
            a = orc.fill_uniform(n, q, 10 + l)
            pk0 = (np.uint64(q) - orc.pointwise(a, cx.fwd(s), q)) % np.uint64(q)
            c0 = (orc.pointwise(pk0, cx.fwd(u), q).astype(object) + cx.fwd(e).astype(object) + cx.fwd(pt).astype(object)) % q
            lines.append("%s c0 limb %d q %d checksum %016x" % (what, l, q, orc.checksum(c0.astype(np.uint64))))
        lines.append("bfv decrypted == message: yes" if what == "bfv" else "ckks decoded == (rint(y Delta) + e) / Delta: yes")
    return lines


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        run_instance(lib, orc, pol, k, logn)
    primes, roots = rs.chain(lib, 1 << 10, [50, 50, 50])
    check_lift(lib, orc, primes, roots, 1 << 10, 2, "plain", 0)
    print("lift launch proof: %d instances driven" % (len(rs.fused_launch_cases()) + 1))


if __name__ == "__main__":
    main()
