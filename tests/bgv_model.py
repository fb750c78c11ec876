"""Model of the BGV ModDown (ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch) for the tests: the definition of
include/ntt_mi355x.h in its own order -- t_j [T^-1]_{p_j}, + [h]_{p_j}, times [p^_j^-1]_{p_j}, the sum mod q_l, - [h]_{q_l}, times
[T]_{q_l}, the difference times [P^-1]_{q_l} -- with the modular products through the oracle's pointwise product and the transforms
through Oracle().ctx (nothing of the kernels' arithmetic, none of their folded constants); a Python-integer form for small sizes; a toy
BGV (encryption, tensor, hybrid relinearisation with ModUp overshoot and key noise T e, modulus switch, decryption) on top of it; the
same multiplication through the library calls (mul_on_device: tests/test_gpu_bgv.py and tests/test_gpu_plain.py run it); the case
runners of tests/test_gpu_bgv.py and the model of examples/rns_bgv_mul.c.
"""
import numpy as np

import ct_mul_model as cm
import keyswitch_model as km
import rns_support as rs

TRANSFORMED, FLOOR, ACCUMULATE = 1, 2, 4
PT = 65537  # the plaintext modulus of the BGV tests
prod = km.prod


def _mul(orc, x, k, q):
    """x * k mod q for an array x of canonical words and an integer k in [0, q)"""
    x = rs.u64(x)
    return orc.pointwise(x, rs.full(x.size, k), q) if k else np.zeros(x.size, dtype=np.uint64)


def subtrahend(orc, pr, t, q, T):
    """[T]_q (F - [h]_q) mod q, canonical, for the P limbs' coefficients t (numpy uint64 arrays)"""
    P = prod(pr)
    h = (P - 1) // 2
    acc = np.zeros(len(t[0]), dtype=np.uint64)
    for p, x in zip(pr, t):
        w = (_mul(orc, x, pow(T % p, -1, p), p) + np.uint64((p - 1) // 2)) % np.uint64(p)  # < 2^62: no wrap
        z = _mul(orc, w, pow(P // p % p, -1, p), p)
        acc = (acc + _mul(orc, z % np.uint64(q), P // p % q, q)) % np.uint64(q)
    return _mul(orc, (acc + np.uint64(q - h % q)) % np.uint64(q), T % q, q)


def word_int(pr, ts, q, c, T):
    """one output word with Python integers: the definition, literally"""
    P = prod(pr)
    h = (P - 1) // 2
    F = 0
    for p, t in zip(pr, ts):
        z = (int(t) * pow(T % p, -1, p) + (p - 1) // 2) * pow(P // p % p, -1, p) % p
        F += z * (P // p % q)
    F %= q
    return (int(c) - (T % q) * (F - h % q)) * pow(P % q, -1, q) % q


def mod_down_bgv(orc, primes, roots, np_, limbs, n, T, flags):
    """the last np_ primes are P.  Returns (Q limbs after the call, the P limbs' slots after the call)"""
    nq = len(primes) - np_
    pr = primes[nq:]
    P = prod(pr)
    t = [orc.ctx(n, p, w).inv(c) if flags & TRANSFORMED else rs.u64(c) for p, w, c in zip(pr, roots[nq:], limbs[nq:])]
    out = []
    for q, w, c in zip(primes[:nq], roots[:nq], limbs[:nq]):
        u = subtrahend(orc, pr, t, q, T)
        if flags & TRANSFORMED:
            u = orc.ctx(n, q, w).fwd(u)  # (linear: the transform of the difference is the difference of the transforms)
        d = (rs.u64(c) + np.uint64(q) - u) % np.uint64(q)
        out.append(_mul(orc, d, pow(P % q, -1, q), q))
    return out, t


def mod_down_bgv_add(orc, primes, roots, np_, c, a, n, T, flags):
    """mod_down_bgv of the accumulator a, then c_l = r_l or, with ACCUMULATE, (c_l + r_l) mod q_l"""
    r, t = mod_down_bgv(orc, primes, roots, np_, a, n, T, flags & TRANSFORMED)
    if flags & ACCUMULATE:
        r = [(rs.u64(cl) + rl) % np.uint64(q) for cl, rl, q in zip(c, r, primes)]
    return r, t


def centred(x, m):
    return x - m if 2 * x > m else x


def definition(x, pr, T):
    """(y, w): w the centred residue of x T^-1 mod P, y = (x - T w) / P"""
    P = prod(pr)
    w = centred(x * pow(T, -1, P) % P, P)
    assert (x - T * w) % P == 0
    return (x - T * w) // P, w


# ---------------------------------------------------------------- edge words

def edge_ts(primes):
    """T in {1, 2, 65537, a T of 61 bits above every prime the plans accept, T = q_0 (so that [T]_{q_0} = 0)}"""
    return [1, 2, 65537, (1 << 60) + 33, primes[0]]


def edge_words(p):
    return [0, 1, (p - 1) // 2, (p + 1) // 2, p - 1]


def plant(coef, primes, nq, n, batch):
    """every combination of the edge words of P limb 0 with c in {0, q - 1} in front of every polynomial; the other P limbs cycle
    through their own edge words"""
    for b in range(batch):
        k = 0
        for e in range(5):
            for cv in range(2):
                for l, q in enumerate(primes):
                    if l < nq:
                        coef[l][b * n + k] = 0 if cv == 0 else q - 1
                    else:
                        coef[l][b * n + k] = edge_words(q)[(e + (l - nq)) % 5]
                k += 1
    return coef


# ---------------------------------------------------------------- a toy BGV in RNS (every product through the oracle's transforms)

class Bgv:
    """BGV over Q = primes[:nq] with special primes P = primes[nq:], hybrid key switching with digits of alpha Q limbs, plaintext modulus
    T.  Polynomials are lists of per-limb arrays of n words."""

    def __init__(self, orc, primes, roots, nq, alpha, n, T, rng):
        self.orc, self.primes, self.roots, self.nq, self.alpha, self.n, self.T, self.rng = orc, primes, roots, nq, alpha, n, T, rng
        self.ctx = [orc.ctx(n, q, w) for q, w in zip(primes, roots)]
        self.s = [rng.choice((-1, 0, 1)) for _ in range(n)]
        self.s_hat = self.fwd(self.small(self.s))

    def small(self, v, limbs=None):
        return [np.array([x % q for x in v], dtype=np.uint64) for q in self.primes[:limbs or len(self.primes)]]

    def fwd(self, p):
        return [c.fwd(x) for c, x in zip(self.ctx, p)]

    def inv(self, p):
        return [c.inv(x) for c, x in zip(self.ctx, p)]

    def mul(self, a, b):
        return [self.orc.pointwise(x, y, q) for x, y, q in zip(a, b, self.primes)]

    def add(self, a, b):
        return [(x + y) % np.uint64(q) for x, y, q in zip(a, b, self.primes)]

    def neg(self, a):
        return [(np.uint64(q) - x) % np.uint64(q) for x, q in zip(a, self.primes)]

    def uniform(self, limbs):
        return [rs.u64([self.rng.randrange(q) for _ in range(self.n)]) for q in self.primes[:limbs]]

    def noise(self):
        return [self.rng.choice((-1, 0, 1)) for _ in range(self.n)]

    def encrypt(self, m):
        """(c0^, c1^) over Q, NTT domain: c0 + c1 s = m + T e"""
        a = self.uniform(self.nq)
        e = self.noise()
        body = self.fwd(self.small([mi + self.T * ei for mi, ei in zip(m, e)], self.nq))
        return self.add(self.neg(self.mul(a, self.s_hat)), body), a

    def relin_keys(self):
        """per digit k: (b_k^, a_k^) over Q u P with b_k + a_k s = T e_k + P Q^_k [Q^_k^-1]_{Q_k} s^2"""
        nl = len(self.primes)
        Q, P = prod(self.primes[:self.nq]), prod(self.primes[self.nq:])
        s2 = self.mul(self.s_hat, self.s_hat)
        keys = []
        for k in range(self.nq // self.alpha):
            Qk = prod(self.primes[self.alpha * k:self.alpha * (k + 1)])
            f = P * (Q // Qk) * pow(Q // Qk % Qk, -1, Qk)
            a = self.uniform(nl)
            te = self.fwd(self.small([self.T * x for x in self.noise()]))
            fs2 = [_mul(self.orc, x, f % q, q) for x, q in zip(s2, self.primes)]
            keys.append((self.add(self.add(self.neg(self.mul(a, self.s_hat)), te), fs2), a))
        return keys

    def decrypt(self, ct, limbs):
        """[sum_i c_i s^i]_Q centred, mod T, over the first `limbs` primes"""
        acc, sp = list(ct[0][:limbs]), None
        for ci in ct[1:]:
            sp = self.s_hat[:limbs] if sp is None else [self.orc.pointwise(x, y, q) for x, y, q in zip(sp, self.s_hat, self.primes)]
            acc = [(x + self.orc.pointwise(y, z, q)) % np.uint64(q) for x, y, z, q in zip(acc, ci[:limbs], sp, self.primes)]
        coef = [c.inv(x) for c, x in zip(self.ctx, acc)]
        Q = prod(self.primes[:limbs])
        return [centred(v, Q) % self.T for v in km.crt(coef, self.primes[:limbs])]

    def plain_product(self, m1, m2):
        """m1 m2 in Z_T[X] / (X^n + 1): the coefficients stay below n T^2 < q_0, so one limb's transform is exact"""
        q = self.primes[0]
        assert self.n * self.T * self.T < q
        a, b = (self.ctx[0].fwd(rs.u64(m)) for m in (m1, m2))
        c = self.ctx[0].inv(self.orc.pointwise(a, b, q))
        return [centred(int(v), q) % self.T for v in c]

    def multiply(self, ct1, ct2, keys):
        """tensor, inverse of d2, per digit the approximate ModUp and both key products, BGV ModDown into (d0, d1), then the switch by
        the last Q prime.  Returns (the switched ciphertext over nq - 1 limbs, the relinearised one over nq limbs, every buffer)"""
        nq, orc, pr, ro, n = self.nq, self.orc, self.primes, self.roots, self.n
        d0, d1, d2 = cm.tensor(orc, pr[:nq], ct1[0], ct1[1], ct2[0], ct2[1])
        d2c = [c.inv(x) for c, x in zip(self.ctx, d2)]
        acc = [[np.zeros(n, dtype=np.uint64) for _ in pr] for _ in range(2)]
        for k, key in enumerate(keys):
            ext = [np.zeros(n, dtype=np.uint64) for _ in pr]
            for l in range(self.alpha * k, self.alpha * (k + 1)):
                ext[l] = d2c[l]
            ext = km.mod_up(orc, pr, ro, ext, n, self.alpha * k, self.alpha, 0)
            x = self.fwd(ext)
            for j in range(2):
                acc[j] = self.add(acc[j], self.mul(x, key[j]))
        relin = [mod_down_bgv_add(orc, pr, ro, len(pr) - nq, d, a, n, self.T, TRANSFORMED | ACCUMULATE)[0] for d, a in zip((d0, d1), acc)]
        switched = [mod_down_bgv(orc, pr[:nq], ro[:nq], 1, c, n, self.T, TRANSFORMED)[0] for c in relin]
        return switched, relin, (d0, d1, d2, acc)


def example_model(lib, orc):
    """{(component, limb): checksum} of examples/rns_bgv_mul.c: examples/rns_ciphertext_mul.c with the BGV ModDown for the approximate
    one and the BGV switch by the last Q prime for the rescale"""
    n, nq, np_, alpha, T = 1 << 13, 8, 2, 2, 65537
    primes, roots = cm.example_primes(lib, n)
    ct = [[orc.fill_uniform(n, q, 100 + 16 * j + l) for l, q in enumerate(primes[:nq])] for j in range(4)]  # a0, a1, b0, b1
    d0, d1, d2 = cm.tensor(orc, primes[:nq], *ct)
    d2c = [orc.ctx(n, q, w).inv(v) for q, w, v in zip(primes, roots, d2)]
    acc = [[np.zeros(n, dtype=np.uint64) for _ in primes] for _ in range(2)]
    for k in range(nq // alpha):
        ext = [np.zeros(n, dtype=np.uint64) for _ in primes]
        for l in range(alpha * k, alpha * (k + 1)):
            ext[l] = d2c[l]
        ext = km.mod_up(orc, primes, roots, ext, n, alpha * k, alpha, 0)
        for l, (q, w) in enumerate(zip(primes, roots)):
            x = orc.ctx(n, q, w).fwd(ext[l])
            for j in range(2):
                key = orc.fill_uniform(n, q, 1000 + 500 * j + 16 * k + l)
                acc[j][l] = (acc[j][l] + orc.pointwise(x, key, q)) % np.uint64(q)
    out = {}
    for j, d in enumerate((d0, d1)):
        c, _ = mod_down_bgv_add(orc, primes, roots, np_, d, acc[j], n, T, TRANSFORMED | ACCUMULATE)
        kept, _ = mod_down_bgv(orc, primes[:nq], roots[:nq], 1, c, n, T, TRANSFORMED)
        for l in range(nq - 1):
            out[(j, l)] = orc.checksum(kept[l])
    return out


# ---------------------------------------------------------------- BGV through the library calls

def _image(polys, n):
    return np.concatenate([np.concatenate([rs.u64(l) for l in p]) for p in polys])


def mul_on_device(lib, bgv, ct1, ct2, keys):
    """the sequence of examples/rns_bgv_mul.c; returns ((d0, d1) after relinearisation, (d0, d1) after the switch) as per-limb arrays"""
    n, nq, nl, alpha, pt = bgv.n, bgv.nq, len(bgv.primes), bgv.alpha, bgv.T
    plans = [lib.Plan(n, q, w) for q, w in zip(bgv.primes, bgv.roots)]
    cp, ap = nq * n, nl * n
    din = lib.DeviceBuffer(4 * cp).upload(_image([ct1[0], ct1[1], ct2[0], ct2[1]], n))
    d, ext, acc = lib.DeviceBuffer(3 * cp), lib.DeviceBuffer(ap).upload(np.zeros(ap, dtype=np.uint64)), lib.DeviceBuffer(2 * ap)
    kbufs = [lib.DeviceBuffer(2 * ap).upload(_image(key, n)) for key in keys]
    try:
        i = [din.ptr + 8 * j * cp for j in range(4)]
        o = [d.ptr + 8 * j * cp for j in range(3)]
        lib.rns_tensor(plans[:nq], o[0], o[1], o[2], i[0], i[1], i[2], i[3], 1, 0, layout=(n, cp))
        lib.rns_inv(plans[:nq], o[2], 1, layout=(n, cp))
        for k, kb in enumerate(kbufs):
            lib.copy_probe(ext.ptr + 8 * alpha * k * n, o[2] + 8 * alpha * k * n, alpha * n)
            lib.rns_mod_up_mul_pair(plans, acc.ptr, acc.ptr + 8 * ap, ext.ptr, alpha * k, alpha, kb.ptr, kb.ptr + 8 * ap, 1,
                                    lib.MUL_B_BROADCAST | (lib.MUL_ACCUMULATE if k else 0), layout=(n, ap))
        lib.rns_mod_down_bgv_add(plans, nl - nq, d.ptr, acc.ptr, pt, 2, TRANSFORMED | ACCUMULATE, layout=(n, cp, n, ap))
        relin = d.download()
        lib.rns_mod_down_bgv(plans[:nq], 1, d.ptr, pt, 2, TRANSFORMED, layout=(n, cp))
        switched = d.download()
    finally:
        for b in [din, d, ext, acc] + kbufs:
            b.free()
        for p in plans:
            p.destroy()
    cut = lambda img, limbs: [[img[j * cp + l * n:j * cp + (l + 1) * n] for l in range(limbs)] for j in range(2)]
    return cut(relin, nq), cut(switched, nq - 1)


# ---------------------------------------------------------------- GPU case runners

def _operand(orc, primes, roots, nq, n, batch, flags, seed, edges=False):
    coef = [orc.fill_uniform(batch * n, q, seed * 1000 + l) for l, q in enumerate(primes)]
    if batch and n >= 16:
        if edges:
            plant(coef, primes, nq, n, batch)
        else:
            for l, q in enumerate(primes):
                rs.edge_fill(coef[l], q)
    return [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & TRANSFORMED else coef


def run_down(lib, orc, primes, roots, np_, n, batch, T, flags, layout="limb", fused=None, seed=1, plans=None, edges=False):
    """one in-place BGV ModDown on random canonical operands (edges: the edge words planted in front of every polynomial's coefficients),
    every word checked against the model (the P slots included).  Returns the Q limbs after the call."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    nq = len(primes) - np_
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_BGV_FUSED, fused)
        limbs = _operand(orc, primes, roots, nq, n, batch, flags, seed, edges)
        got = km._call(lib, lambda ptr, lay: lib.rns_mod_down_bgv(plans, np_, ptr, T, batch, flags, layout=lay), primes, n, batch, limbs, layout)
    finally:
        if fused is not None:
            plans[0].set_option(lib.OPT_BGV_FUSED, -1)
        if own:
            for p in plans:
                p.destroy()
    want, t = mod_down_bgv(orc, primes, roots, np_, limbs, n, T, flags)
    what = "(N=%d, batch %d, np %d, T %d, flags %d, %s, fused %s)" % (n, batch, np_, T, flags, layout, fused)
    for l in range(nq):
        assert np.array_equal(got[l], want[l]), "Q limb %d of %d differs from the model %s" % (l, nq, what)
    for j in range(np_):
        assert np.array_equal(got[nq + j], t[j] if flags & TRANSFORMED else limbs[nq + j]), "P slot %d %s" % (j, what)
    return got[:nq]


def run_down_add(lib, orc, primes, roots, np_, n, batch, T, flags, c_layout="limb", a_layout="limb", fused=None, seed=1, plans=None,
                 a_untouched=None, edges=False):
    """one BGV ModDown into a ciphertext: every word of the ciphertext against the model; the accumulator's P slots; its Q limbs unchanged
    where a_untouched; canaries around both operands.  Returns the ciphertext's limbs."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    nq = len(primes) - np_
    dom = flags & TRANSFORMED
    a = _operand(orc, primes, roots, nq, n, batch, dom, seed, edges)
    c = km._operand(orc, primes[:nq], roots[:nq], n, batch, dom, seed + 50)
    ia, ic = cm._Image(lib, a, n, batch, a_layout), cm._Image(lib, c, n, batch, c_layout)
    lay = None if (c_layout, a_layout) == ("limb", "limb") else (ic.ls, ic.ps, ia.ls, ia.ps)
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_BGV_FUSED, fused)
        lib.rns_mod_down_bgv_add(plans, np_, ic.ptr, ia.ptr, T, batch, flags, layout=lay)
        got, after = ic.limbs(), ia.limbs()
    finally:
        if fused is not None:
            plans[0].set_option(lib.OPT_BGV_FUSED, -1)
        ia.free(), ic.free()
        if own:
            for p in plans:
                p.destroy()
    want, t = mod_down_bgv_add(orc, primes, roots, np_, c, a, n, T, flags)
    what = "(N=%d, batch %d, nq %d, np %d, T %d, flags %d, c %s, a %s, fused %s)" % (n, batch, nq, np_, T, flags, c_layout, a_layout, fused)
    for l in range(nq):
        assert np.array_equal(got[l], want[l]), "limb %d differs from the model %s" % (l, what)
    for j in range(np_):
        assert np.array_equal(after[nq + j], t[j] if dom else a[nq + j]), "P slot %d %s" % (j, what)
    if a_untouched:
        for l in range(nq):
            assert np.array_equal(after[l], a[l]), "the accumulator's Q limb %d was written %s" % (l, what)
    return got
