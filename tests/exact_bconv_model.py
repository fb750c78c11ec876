"""Model of the exact RNS base conversion and the exact scaled ModDown (ntt_rns_mod_up_exact_batch, ntt_rns_mod_down_exact_batch) for the
tests: the formulas of include/ntt_mi355x.h with the integer sums reduced through the oracle's pointwise product (Python integers in
the *_int forms) and the floating-point sum s in numpy.float64, in the header's operation order -- fl(z_i) * rho_i added left to
right, rint to even; the transforms through Oracle().ctx (nothing of the kernels' arithmetic).  A toy BFV (encryption, the four-step
tensor-and-scale, decryption) on top of the two primitives, the same four steps through the library calls (bfv_on_device:
tests/test_gpu_exact_bconv.py and tests/test_gpu_plain.py run it), and the case runners of tests/test_gpu_exact_bconv.py.
"""
import numpy as np

import ct_mul_model as cm
import keyswitch_model as km
import rns_support as rs

TRANSFORMED, FLOOR, ACCUMULATE = 1, 2, 4
prod = km.prod


def digits(orc, basis, words, mult=1):
    """z_i = [x_i * mult * b^_i^-1]_{b_i} per source prime (numpy uint64)"""
    B = prod(basis)
    return [orc.pointwise(rs.u64(x), rs.full(len(x), mult % b * pow(B // b % b, -1, b) % b), b) for b, x in zip(basis, words)]


def correction(basis, z):
    """v = rint(s), s = ((fl(z_0) rho_0 + fl(z_1) rho_1) + ...), rho_i = 1.0 / (double)b_i: every operation one IEEE double operation"""
    s = None
    for b, zi in zip(basis, z):
        term = zi.astype(np.float64) * (np.float64(1.0) / np.float64(b))
        s = term if s is None else s + term
    return np.rint(s).astype(np.uint64)


def exact_bconv(orc, basis, words, q, mult=1):
    """ExactBConv_{B->q}([mult x]_B) = ( sum_i z_i [b^_i]_q - v [B]_q ) mod q for the words x_i canonical mod b_i.  Returns (the
    conversion, v)."""
    B = prod(basis)
    z = digits(orc, basis, words, mult)
    v = correction(basis, z)
    acc = np.zeros(len(z[0]), dtype=np.uint64)
    for b, zi in zip(basis, z):
        acc = (acc + orc.pointwise(zi % np.uint64(q), rs.full(zi.size, B // b % q), q)) % np.uint64(q)  # < 2^62: no wrap
    return (acc + orc.pointwise(v, rs.full(v.size, q - B % q), q)) % np.uint64(q), v


def exact_bconv_int(basis, words, q, mult=1):
    """the same with Python integers for the sums, one coefficient at a time (small sizes)"""
    B = prod(basis)
    z = [[int(x) * (mult % b * pow(B // b % b, -1, b) % b) % b for x in xs] for b, xs in zip(basis, words)]
    v = correction(basis, [np.array(zi, dtype=np.uint64) for zi in z])
    return [(sum(zi[k] * (B // b) for b, zi in zip(basis, z)) - int(v[k]) * B) % q for k in range(len(words[0]))], v


def mod_up_exact(orc, primes, roots, limbs, n, first, count, flags):
    """limbs: the operand's arrays (batch * n words each) in the call's domain.  Returns every limb after the call."""
    basis = primes[first:first + count]
    coef = [orc.ctx(n, primes[i], roots[i]).inv(limbs[i]) if flags & TRANSFORMED else rs.u64(limbs[i]) for i in range(first, first + count)]
    out = []
    for l, (q, w) in enumerate(zip(primes, roots)):
        if first <= l < first + count:
            out.append(rs.u64(limbs[l]))
            continue
        v, _ = exact_bconv(orc, basis, coef, q)
        out.append(orc.ctx(n, q, w).fwd(v) if flags & TRANSFORMED else v)
    return out


def mod_down_exact(orc, primes, roots, np_, limbs, n, mult, flags):
    """the last np_ primes are P.  c_l <- c_l [mult P^-1] - ExactBConv_{P->q_l}([mult t]_P) [P^-1]  (mod q_l).  Returns (Q limbs after
    the call, the P limbs' slots after the call)"""
    nq = len(primes) - np_
    pr = primes[nq:]
    P = prod(pr)
    t = [orc.ctx(n, p, w).inv(c) if flags & TRANSFORMED else rs.u64(c) for p, w, c in zip(pr, roots[nq:], limbs[nq:])]
    out = []
    for q, w, c in zip(primes[:nq], roots[:nq], limbs[:nq]):
        u, _ = exact_bconv(orc, pr, t, q, mult)
        c = orc.ctx(n, q, w).inv(c) if flags & TRANSFORMED else rs.u64(c)
        pinv = pow(P % q, -1, q)
        a = orc.pointwise(c, rs.full(c.size, mult % q * pinv % q), q)
        b = orc.pointwise(u, rs.full(u.size, pinv), q)
        r = (a + np.uint64(q) - b) % np.uint64(q)
        out.append(orc.ctx(n, q, w).fwd(r) if flags & TRANSFORMED else r)
    return out, t


def centred(x, B):
    return x - B if 2 * x > B else x


def outside_band(x, B):
    """|2x - B| > 2^-43 B: where the result is fixed by the header's error bound"""
    return abs(2 * x - B) << 43 > B


# ---------------------------------------------------------------- a toy BFV over the two primitives

def negacyclic(a, b, n, mod):
    """a b in Z_mod[X] / (X^n + 1), Python integers"""
    c = [0] * n
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                c[k] += x * y
            else:
                c[k - n] -= x * y
    return [v % mod for v in c]


def bfv_keygen(rng, n):
    return [rng.choice((-1, 0, 1)) for _ in range(n)]


def bfv_encrypt(rng, s, m, n, Q, t):
    """(c0, c1) with c0 + c1 s = floor(Q / t) m + e (mod Q), e ternary"""
    a = [rng.randrange(Q) for _ in range(n)]
    e = [rng.choice((-1, 0, 1)) for _ in range(n)]
    as_ = negacyclic(a, s, n, Q)
    return [(Q // t * mi + ei - x) % Q for mi, ei, x in zip(m, e, as_)], a


def bfv_decrypt(s, d, n, Q, t):
    """round(t / Q * [d0 + d1 s + d2 s^2]_Q centred) mod t"""
    ph, sp = list(d[0]), list(s)
    for di in d[1:]:
        ph = [(x + y) % Q for x, y in zip(ph, negacyclic(di, sp, n, Q))]
        sp = [centred(v, Q) for v in negacyclic(sp, s, n, Q)]
    return [((2 * t * centred(x, Q) + Q) // (2 * Q)) % t for x in ph]


def bfv_mul(orc, primes, roots, nr, t, a0, a1, b0, b1, n):
    """the five calls of examples/rns_bfv_mul.c on the model: primes = R (nr of them) then Q; a0, a1, b0, b1 the operands' Q limbs in the
    NTT domain (lists of nq arrays of n words).  Returns (d0, d1, d2)'s Q limbs in the NTT domain and the buffers after every step."""
    nq = len(primes) - nr
    ins = []
    for p in (a0, a1, b0, b1):
        ext = mod_up_exact(orc, primes, roots, [np.zeros(n, dtype=np.uint64)] * nr + list(p), n, nr, nq, TRANSFORMED)
        ins.append(ext)
    d = cm.tensor(orc, primes, *ins)
    # R first: the ModDown keeps R (slots 0 .. nr-1), divides by Q and leaves Q's coefficients in slots nr ..
    scaled = [mod_down_exact(orc, primes, roots, nq, di, n, t, TRANSFORMED) for di in d]
    back = [mod_up_exact(orc, primes, roots, list(r) + list(tq), n, 0, nr, TRANSFORMED) for r, tq in scaled]
    return [b[nr:] for b in back], (ins, d, scaled, back)


def example_model(lib, orc):
    """{(component, Q limb): checksum} of examples/rns_bfv_mul.c"""
    n, nr, nq, t = 1 << 13, 5, 4, 65537
    primes, roots = rs.chain(lib, n, [50] * (nr + nq))
    ct = [[orc.fill_uniform(n, q, 100 + 16 * j + l) for l, q in enumerate(primes) if l >= nr] for j in range(4)]  # a0, a1, b0, b1
    d, _ = bfv_mul(orc, primes, roots, nr, t, *ct, n)
    return {(j, l): orc.checksum(d[j][l]) for j in range(3) for l in range(nq)}


# ---------------------------------------------------------------- BFV through the library calls

def bfv_on_device(lib, primes, roots, nr, t, ct_ntt, n):
    """the example's four calls on [4][nr + nq][n] / [3][nr + nq][n] buffers; returns the three result polynomials' limbs"""
    nl = len(primes)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    poly = nl * n
    img = np.zeros(4 * poly, dtype=np.uint64)
    for j, p in enumerate(ct_ntt):
        for l, c in enumerate(p):
            img[j * poly + (nr + l) * n:j * poly + (nr + l + 1) * n] = c
    din, d = lib.DeviceBuffer(4 * poly).upload(img), lib.DeviceBuffer(3 * poly)
    try:
        lay = (n, poly)
        lib.rns_mod_up_exact(plans, din.ptr, nr, nl - nr, 4, TRANSFORMED, layout=lay)
        o = [d.ptr + 8 * j * poly for j in range(3)]
        i = [din.ptr + 8 * j * poly for j in range(4)]
        lib.rns_tensor(plans, o[0], o[1], o[2], i[0], i[1], i[2], i[3], 1, 0, layout=lay)
        lib.rns_mod_down_exact(plans, nl - nr, d.ptr, t, 3, TRANSFORMED, layout=lay)
        lib.rns_mod_up_exact(plans, d.ptr, 0, nr, 3, TRANSFORMED, layout=lay)
        out = d.download()
    finally:
        din.free(), d.free()
        for p in plans:
            p.destroy()
    return [[out[j * poly + l * n:j * poly + (l + 1) * n] for l in range(nl)] for j in range(3)]


# ---------------------------------------------------------------- GPU case runners

def band_words(basis, k):
    """the RNS words of (B - 1) / 2 and (B + 1) / 2 alternately, k of them: |2x - B| = 1"""
    B = prod(basis)
    xs = [(B - 1) // 2 if i % 2 == 0 else (B + 1) // 2 for i in range(k)]
    return km.residues(xs, basis)


def _operand(orc, primes, roots, n, batch, flags, seed, plant=None):
    """random canonical coefficients with the extremes of the range in front; plant = (first limb, count): the words of (B -+ 1) / 2 of
    that basis in coefficients 4 .. 7 of every polynomial"""
    coef = [orc.fill_uniform(batch * n, q, seed * 1000 + l) for l, q in enumerate(primes)]
    if batch and n >= 8:
        for l, q in enumerate(primes):
            rs.edge_fill(coef[l], q)
        if plant:
            words = band_words(primes[plant[0]:plant[0] + plant[1]], 4)
            for i, w in enumerate(words):
                for p in range(batch):
                    coef[plant[0] + i][p * n + 4:p * n + 8] = w
    return [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & TRANSFORMED else coef


def run_up(lib, orc, primes, roots, first, count, n, batch, flags, layout="limb", seed=1, plans=None, band=False):
    """one exact ModUp on random canonical operands (band: (B -+ 1) / 2 planted in the digit), every word checked against the model.
    Returns the limbs after the call."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    try:
        limbs = _operand(orc, primes, roots, n, batch, flags, seed, (first, count) if band else None)
        got = km._call(lib, lambda ptr, lay: lib.rns_mod_up_exact(plans, ptr, first, count, batch, flags, layout=lay), primes, n, batch,
                       limbs, layout)
    finally:
        if own:
            for p in plans:
                p.destroy()
    want = mod_up_exact(orc, primes, roots, limbs, n, first, count, flags)
    for l in range(len(primes)):
        assert np.array_equal(got[l], want[l]), "limb %d of %d differs from the model (N=%d, batch %d, digit [%d, %d), flags %d, %s)" % (
            l, len(primes), n, batch, first, first + count, flags, layout)
    return got


def run_down(lib, orc, primes, roots, np_, n, batch, mult, flags, layout="limb", fused=None, seed=1, plans=None, band=False):
    """one exact ModDown on random canonical operands (band: (P -+ 1) / 2 planted in the P limbs; mult = 1 keeps them there), every word
    checked against the model (the P slots included).  Returns the Q limbs after the call."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    nq = len(primes) - np_
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
        limbs = _operand(orc, primes, roots, n, batch, flags, seed, (nq, np_) if band else None)
        got = km._call(lib, lambda ptr, lay: lib.rns_mod_down_exact(plans, np_, ptr, mult, batch, flags, layout=lay), primes, n, batch,
                       limbs, layout)
    finally:
        if own:
            for p in plans:
                p.destroy()
    want, t = mod_down_exact(orc, primes, roots, np_, limbs, n, mult, flags)
    for l in range(nq):
        assert np.array_equal(got[l], want[l]), "Q limb %d of %d differs from the model (N=%d, batch %d, np %d, mult %d, flags %d, %s)" % (
            l, nq, n, batch, np_, mult, flags, layout)
    for j in range(np_):
        assert np.array_equal(got[nq + j], t[j] if flags & TRANSFORMED else limbs[nq + j]), "P slot %d" % j
    return got[:nq]
