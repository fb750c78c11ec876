"""Model of the device-side sampler (ntt_rns_sample_batch) for the tests: Philox4x32-10 and the three kinds of
csrc/ntt_sample.h in vectorised numpy, and the GPU case runner.  The definition fixes every output word: the comparisons are bit for
bit, there is no band and no tolerance.

Script mode (`python3 tests/sample_model.py`, a fresh process under a kernel trace): one call per sampling kernel instance -- every
sample_fwd_kernel (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W) and sample_coef_kernel -- each checked against the model
(the launch proof); `--route`: one NTT-domain call at 2^14 over 17 FP64 limbs with the fused kernel selected (the route proof).
"""
import sys

import numpy as np

import rns_support as rs

TERNARY, CBD21, UNIFORM = 0, 1, 2
TRANSFORMED, ACCUMULATE = 2, 4
KINDS = [TERNARY, CBD21, UNIFORM]
KIND_IDS = ["ternary", "cbd21", "uniform"]
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1
MULTS = [1, 65537, (1 << 61) - 1]


# ---------------------------------------------------------------- the definition

def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64: the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)  # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def tag_of(kind, l=0):
    return (2 | (l << 8)) if kind == UNIFORM else kind


def blocks_at(seed, Ps, ss, tag):
    """the blocks of the (polynomial, position) pairs (Ps[i], ss[i])"""
    Ps = np.array([int(P) & MASK64 for P in Ps], dtype=np.uint64)
    return philox(np.asarray(ss, dtype=np.uint64), Ps & np.uint64(MASK32), Ps >> np.uint64(32), np.full(Ps.size, tag, dtype=np.uint64),
                  seed & MASK32, (seed >> 32) & MASK32)


def blocks(seed, P, n, tag):
    """the blocks of positions 0..n-1 of polynomial P"""
    return blocks_at(seed, [P] * n, np.arange(n, dtype=np.uint64), tag)


def popcount21(x):
    x = x & np.uint64(0x1FFFFF)
    return sum(((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64) for b in range(21))


def small_of(kind, o0, o1):
    """the centred values (int64) of blocks with the words o0, o1"""
    if kind == CBD21:
        return popcount21(o0) - popcount21(o1)
    # mulhi64(w, 3) for w = o0 | o1 << 32: floor((3 o1 2^32 + 3 o0) / 2^64) = (3 o1 + (3 o0 >> 32)) >> 32, every term below 2^35
    return (((np.uint64(3) * o1 + ((np.uint64(3) * o0) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)) - 1


def uniform_of(o0, o1, o2, o3, q):
    """the 128-bit blocks mod q (Python integers: exact)"""
    lo, hi = o0 | (o1 << np.uint64(32)), o2 | (o3 << np.uint64(32))
    return np.array([((int(h) << 64) | int(w)) % q for h, w in zip(hi, lo)], dtype=np.uint64)


def small(kind, seed, P, n):
    """the centred values (int64) of positions 0..n-1 of polynomial P"""
    o0, o1, _, _ = blocks(seed, P, n, kind)
    return small_of(kind, o0, o1)


def uniform(seed, P, n, l, q):
    """positions 0..n-1 of polynomial P, limb index l of the call, mod q"""
    return uniform_of(*blocks(seed, P, n, tag_of(UNIFORM, l)), q)


def small_table(mult, q):
    """[mult v]_q for v = -21..21 (index v + 21)"""
    return np.array([(v * mult) % q for v in range(-21, 22)], dtype=np.uint64)


def sample(kind, primes, n, batch, seed, first_poly=0, mult=1):
    """[limb] arrays of canonical words, [batch][N] each: the definition"""
    out = []
    vs = None if kind == UNIFORM else [small(kind, seed, first_poly + p, n) for p in range(batch)]
    for l, q in enumerate(primes):
        if kind == UNIFORM:
            out.append(np.concatenate([uniform(seed, first_poly + p, n, l, q) for p in range(batch)]))
        else:
            out.append(np.concatenate([small_table(mult, q)[vp + 21] for vp in vs]))
    return out


def centred(words, q):
    """canonical words back to the centred integers (int64)"""
    w = np.asarray(words, dtype=np.uint64)
    return np.where(w > np.uint64(q // 2), w.astype(np.int64) - np.int64(q), w.astype(np.int64))


# ---------------------------------------------------------------- GPU case runner

CANARY = 0xC0FFEE11F7ED0B5E


def expected(orc, kind, primes, roots, n, batch, seed, first_poly, mult, flags, acc_in=None):
    """the output limbs: the definition, through the oracle's forward transform with TRANSFORMED (the small kinds), added to acc_in with
    ACCUMULATE"""
    out = sample(kind, primes, n, batch, seed, first_poly, mult)
    if flags & TRANSFORMED and kind != UNIFORM:
        out = [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, out)]
    if flags & ACCUMULATE:
        out = [((a.astype(object) + c.astype(object)) % q).astype(np.uint64) for a, c, q in zip(acc_in, out, primes)]
    return out


def check_sample(lib, orc, primes, roots, n, batch, kind, flags=0, seed=0x5EED, first_poly=0, mult=1, layout="limb", fused=None,
                 max_grid=None, arith=None, plans=None):
    """one call, checked word for word.  The output (layout: rns_support's kinds) sits among canaries (64 words either side and in
    every gap), which must stay untouched.  Without ACCUMULATE the output slots start as canaries too: every word must be written; with
    it they hold uniform words whose first four are the edges of the canonical range.  Returns the output limbs."""
    nl, pad = len(primes), 64
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w, **({"arith": arith} if arith else {})) for q, w in zip(primes, roots)]
    if fused is not None:
        plans[0].set_option(lib.OPT_SAMPLE_FUSED, fused)
    if max_grid is not None:
        for p in plans:
            p.set_option(lib.OPT_MAX_GRID, max_grid)
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    acc_in = None
    if flags & ACCUMULATE:
        acc_in = [orc.fill_uniform(batch * n, q, 977 + l) for l, q in enumerate(primes)]
        if batch * n >= 4:
            for a, q in zip(acc_in, primes):
                rs.edge_fill(a, q)
    img_c = rs.place(acc_in, n, batch, ls, ps, words) if acc_in is not None else np.full(words, rs.CANARY, dtype=np.uint64)
    host_c = np.concatenate([np.full(pad, CANARY, dtype=np.uint64), img_c, np.full(pad, CANARY, dtype=np.uint64)])
    dc = lib.DeviceBuffer(host_c.size).upload(host_c)
    try:
        lib.rns_sample(plans, dc.ptr + 8 * pad, kind, seed, batch, first_poly=first_poly, mult=mult, flags=flags,
                       layout=None if layout == "limb" else (ls, ps))
        got_c = dc.download()
    finally:
        dc.free()
        if fused is not None:
            plans[0].set_option(lib.OPT_SAMPLE_FUSED, -1)
        if own:
            for p in plans:
                p.destroy()
    assert np.array_equal(got_c[:pad], host_c[:pad]) and np.array_equal(got_c[-pad:], host_c[-pad:]), "a word around the output changed"
    got, used = rs.extract(got_c[pad:-pad], nl, n, batch, ls, ps)
    assert np.array_equal(got_c[pad:-pad][~used], img_c[~used]), "a word in a gap of the output changed"
    want = expected(orc, kind, primes, roots, n, batch, seed, first_poly, mult, flags, acc_in)
    for l in range(nl):
        bad = np.nonzero(got[l] != want[l])[0]
        assert bad.size == 0, "limb %d of %d (N=%d, batch %d, kind %d, flags %d, %s): words %s got %s want %s" % (
            l, nl, n, batch, kind, flags, layout, bad[:6].tolist(), got[l][bad[:6]].tolist(), want[l][bad[:6]].tolist())
    return got


def instance_case(logn):
    """(kind, flags, mult) for the per-instance cases: kind, multiplier and accumulation rotate with logn"""
    kind, mult = [(TERNARY, 1), (CBD21, 65537), (CBD21, (1 << 61) - 1)][logn % 3]
    return kind, TRANSFORMED | (ACCUMULATE if (logn // 3) % 2 else 0), mult


def run_instance(lib, orc, pol, k, logn, **kw):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [rs.CLASS_BITS[(pol, k)]] * 3)
    kind, flags, mult = instance_case(logn)
    return check_sample(lib, orc, primes, roots, n, 3 if logn < 9 else 2, kind, flags, seed=logn, first_poly=(1 << 32) - 1, mult=mult,
                        fused=1, **kw)


def route(lib, orc):
    """2^14, 17 limbs of 50-bit primes (two runs of the FP64 policy: 16 + 1), NTT domain, 2 polynomials, the fused kernel selected
    (NTT_OPT_SAMPLE_FUSED 1): the route proof's call"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, [50] * 17)
    check_sample(lib, orc, primes, roots, n, 2, CBD21, TRANSFORMED, fused=1, seed=17)
    print("sample route: one call at 2^14 over 17 limbs")


# ---------------------------------------------------------------- the example

EX_LOGN, EX_T, EX_L, EX_SEED = 12, 65537, 3, 0x5EED


def example_model(lib, orc):
    """the lines examples/rns_sample.c prints: per limb the checksums of the secret s^, the public key (b^, a^) and the ciphertext
    (c0^, c1^) of a BFV encryption whose every random polynomial comes from the sampler, then the decryption's verdict.
    first_poly: s 0, a 1, e 2, u 3, e0 4, e1 5."""
    from lift_model import SCALED, lift
    n, t = 1 << EX_LOGN, EX_T
    primes, roots = rs.chain(lib, n, [50] * EX_L)
    m = orc.fill_uniform(n, t, 1)
    pt = lift(SCALED, m, primes, t)
    s, e, u, e0, e1 = (sample(k, primes, n, 1, EX_SEED, P) for k, P in ((TERNARY, 0), (CBD21, 2), (TERNARY, 3), (CBD21, 4), (CBD21, 5)))
    a = sample(UNIFORM, primes, n, 1, EX_SEED, 1)
    lines = []
    for l, q in enumerate(primes):
        cx = orc.ctx(n, q, roots[l])
        add = lambda x, y: ((x.astype(object) + y.astype(object)) % q).astype(np.uint64)
        sh, uh = cx.fwd(s[l]), cx.fwd(u[l])
        b = add((np.uint64(q) - orc.pointwise(a[l], sh, q)) % np.uint64(q), cx.fwd(e[l]))
        c0 = add(add(orc.pointwise(b, uh, q), cx.fwd(e0[l])), cx.fwd(pt[l]))
        c1 = add(orc.pointwise(a[l], uh, q), cx.fwd(e1[l]))
        lines.append("limb %d q %d s %016x b %016x a %016x c0 %016x c1 %016x" % (
            l, q, orc.checksum(sh), orc.checksum(b), orc.checksum(a[l]), orc.checksum(c0), orc.checksum(c1)))
    lines.append("bfv decrypted == message: yes")
    return lines


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        run_instance(lib, orc, pol, k, logn)
    primes, roots = rs.chain(lib, 1 << 10, [50, 50, 50])
    check_sample(lib, orc, primes, roots, 1 << 10, 2, UNIFORM)
    print("sample launch proof: %d instances driven" % (len(rs.fused_launch_cases()) + 1))


if __name__ == "__main__":
    main()
