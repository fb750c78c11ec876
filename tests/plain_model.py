"""Out of the RNS (ntt_rns_to_plain_batch, ntt_rns_to_double_batch): the two integer definitions in Python integers, the formula of
csrc/ntt_plain.h with its FP64 sum in numpy.float64 in the header's order (what the kernel must reproduce bit for bit), the model of
to_double, and the case runners of the GPU tests."""
from math import gcd, prod

import numpy as np

SCALE = 1  # NTT_PLAIN_SCALE


# ---------------------------------------------------------------- the definitions

def centred(x, Q):
    """the centred representative of x mod Q: x, or x - Q from Q / 2 on (Q odd: no tie)"""
    return x - Q if 2 * x >= Q else x


def definition(x, Q, t, flags=0):
    """default: [x_c]_t; SCALE: round(t x / Q) mod t (Q odd: no ties)"""
    if flags & SCALE:
        return ((2 * t * x + Q) // (2 * Q)) % t
    return centred(x, Q) % t


def in_band(x, Q, t, flags=0):
    """the words the header leaves to the FP64 sum's rounding: |2 rho - Q| <= 2^-43 Q, rho = x (default) or t x mod Q (SCALE)"""
    rho = (t * x) % Q if flags & SCALE else x
    return abs(2 * rho - Q) << 43 <= Q


def neighbours(x, Q, t, flags=0):
    """what a word inside the band may be"""
    if flags & SCALE:
        f = (t * x) // Q
        return {f % t, (f + 1) % t}
    return {x % t, (x - Q) % t}


def to_rns(xs, primes):
    """[limb] arrays of the residues of the integers xs"""
    return [np.array([x % q for x in xs], dtype=np.uint64) for q in primes]


def from_rns(limbs, primes):
    """the integers in [0, Q) behind [limb] arrays of canonical words (big-integer CRT)"""
    Q = prod(primes)
    hats = [(Q // q) * pow(Q // q, -1, q) for q in primes]
    return [sum(int(w) * h for w, h in zip(ws, hats)) % Q for ws in zip(*limbs)]


# ---------------------------------------------------------------- the formula (csrc/ntt_plain.h)

def constants(primes, t, flags=0):
    """(c_i, g_i, rho_i, h): z_i = [x_i c_i]_{q_i}, m = (sum z_i g_i + v h) mod t, v = rint(sum fl(z_i) rho_i)"""
    Q = prod(primes)
    c = [pow(Q // q, -1, q) for q in primes]
    rho = [np.float64(1.0) / np.float64(q) for q in primes]
    if flags & SCALE:
        assert all(gcd(t, q) == 1 for q in primes)
        return [ci * t % q for ci, q in zip(c, primes)], [t - pow(q, -1, t) for q in primes], rho, 1
    return c, [(Q // q) % t for q in primes], rho, (-Q) % t


def formula(limbs, primes, t, flags=0):
    """one output word per coefficient from [limb] arrays of canonical words: the header's statement, every FP64 operation one
    numpy.float64 operation in its order (conversion, product, then the sum left to right, rint to even)"""
    c, g, rho, h = constants(primes, t, flags)
    z = [(np.asarray(x, dtype=np.uint64).astype(object) * ci) % q for x, ci, q in zip(limbs, c, primes)]
    s = None
    for zi, r in zip(z, rho):
        term = zi.astype(np.uint64).astype(np.float64) * r
        s = term if s is None else s + term
    v = np.rint(s).astype(np.uint64).astype(object)
    assert int(v.max()) <= len(primes)
    total = v * h
    for zi, gi in zip(z, g):
        total = total + zi * gi
    assert all(int(w) < (1 << 126) + (1 << 65) for w in total)
    return (total % t).astype(np.uint64)


# ---------------------------------------------------------------- to_double

def double_model(limbs, primes, scale):
    """fl(x_c) * scale as uint64 bit patterns: Python's int -> float is correctly rounded, then one IEEE product"""
    Q = prod(primes)
    y = np.array([np.float64(float(centred(x, Q))) * np.float64(scale) for x in from_rns(limbs, primes)], dtype=np.float64)
    return y.view(np.uint64)


# ---------------------------------------------------------------- corners

def double_values(Q):
    """x mod Q for the x_c of the issue that fit: -+(2^53 + 1), -+(2^53 + 3), 2^100 + 2^47 (+ 1), 0, -+(Q - 1) / 2, -+1"""
    xc = [0, 1, -1, (Q - 1) // 2, -((Q - 1) // 2)]
    for v in (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 100 + 2 ** 47, 2 ** 100 + 2 ** 47 + 1, 2 ** 64, 2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1):
        if 2 * v < Q:
            xc += [v, -v]
    return [v % Q for v in xc]


def corner_values(Q, t, flags=0):
    """x in {0, 1, Q - 1, (Q - 1) / 2, (Q + 1) / 2}; SCALE: the x with t x mod Q = (Q -+ 1) / 2 and the x nearest k Q / t, k = 1, t - 1"""
    xs = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2]
    if flags & SCALE:
        ti = pow(t, -1, Q)
        xs += [((Q - 1) // 2) * ti % Q, ((Q + 1) // 2) * ti % Q]
        for k in (1, t - 1):
            xs += [(k * Q) // t, (k * Q) // t + 1]
    return [x % Q for x in xs]


# ---------------------------------------------------------------- GPU case runners

CANARY = 0xC0FFEE0DDBA11AD5


def _place(limbs, n, batch, ls, ps, words):
    """the [limb][batch * n] words at strides (ls, ps) inside `words` canaries"""
    buf = np.full(words, CANARY, dtype=np.uint64)
    for l, x in enumerate(limbs):
        for p in range(batch):
            buf[l * ls + p * ps:l * ls + p * ps + n] = x[p * n:(p + 1) * n]
    return buf


def run_plain(lib, primes, roots, n, batch, t, flags, limbs, layout=None, alias=False, plans=None, double_scale=None):
    """ntt_rns_to_plain_batch (double_scale: ntt_rns_to_double_batch) on [limb] arrays of batch * n words: the inputs and the output sit
    among canaries (64 words either side, and in every gap of a strided layout), which must stay untouched, as the inputs must --
    except limb 0's slots where the output is the source (alias).  layout = (a_limb_stride, a_poly_stride, m_poly_stride).  Returns
    the batch * n output words (to_double: bit patterns)."""
    nl, pad = len(primes), 64
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    ls, ps, ms = layout if layout else (batch * n, n, n)
    a_words = (nl - 1) * ls + (batch - 1) * ps + n
    m_words = (batch - 1) * ms + n
    host_a = np.concatenate([np.full(pad, CANARY, dtype=np.uint64), _place(limbs, n, batch, ls, ps, a_words), np.full(pad, CANARY, dtype=np.uint64)])
    da = lib.DeviceBuffer(host_a.size).upload(host_a)
    if alias:
        assert ms == ps
        dm, host_m = da, host_a
    else:
        host_m = np.full(m_words + 2 * pad, CANARY, dtype=np.uint64)
        dm = lib.DeviceBuffer(host_m.size).upload(host_m)
    try:
        args = (plans, dm.ptr + 8 * pad, da.ptr + 8 * pad)
        if double_scale is None:
            lib.rns_to_plain(*args, t, batch, flags, layout=layout)
        else:
            lib.rns_to_double(*args, double_scale, batch, layout=layout)
        got_m, got_a = dm.download(), da.download()
    finally:
        da.free()
        if not alias:
            dm.free()
        if own:
            for p in plans:
                p.destroy()
    out = np.concatenate([got_m[pad + p * ms:pad + p * ms + n] for p in range(batch)])
    # everything but the output words is as it was
    want_m = host_m.copy()
    for p in range(batch):
        want_m[pad + p * ms:pad + p * ms + n] = out[p * n:(p + 1) * n]
    assert np.array_equal(got_m, want_m), "words outside the output changed"
    if not alias:
        assert np.array_equal(got_a, host_a), "the source changed"
    return out


def check_plain(lib, primes, roots, n, batch, t, flags, limbs, **kw):
    """run_plain against the formula, bit for bit; returns the words"""
    got = run_plain(lib, primes, roots, n, batch, t, flags, limbs, **kw)
    want = formula(limbs, primes, t, flags)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    return got


def random_limbs(primes, count, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, q, size=count, dtype=np.uint64) for q in primes]


def example_model(lib, orc):
    """the lines examples/rns_decrypt.c prints: the phase is Delta m + e exactly, the plaintext the message"""
    import rns_support as rs
    n, t = 1 << 13, 65537
    primes, _ = rs.chain(lib, n, [50] * 4)
    delta = prod(primes) // t
    m, e = orc.fill_uniform(n, t, 1), orc.fill_uniform(n, 2, 2)
    lines = []
    for l, q in enumerate(primes):
        phase = ((m.astype(object) * (delta % q) + e.astype(object)) % q).astype(np.uint64)
        lines.append("phase limb %d q %d checksum %016x" % (l, q, orc.checksum(phase)))
    assert formula(to_rns([delta * int(a) + int(b) for a, b in zip(m, e)], primes), primes, t, SCALE).tolist() == m.tolist()
    return lines + ["plaintext t %d checksum %016x" % (t, orc.checksum(m)), "decrypted == message: yes"]
