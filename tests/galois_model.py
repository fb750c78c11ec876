"""Model of the Galois automorphisms sigma_g: a(X) -> a(X^g) and of the rotation key product (ntt_galois_batch, ntt_rns_galois_batch,
ntt_rns_galois_dot_batch) for the tests: the two permutations of include/ntt_mi355x.h in numpy (nothing of the kernels' index
functions: bit reversal by loops, the inverse of g by pow), the dot through the oracle's pointwise product (Oracle.dot); the case
runners of tests/test_gpu_galois.py, which place every operand in its layout among canaries and check the output word for word and
the inputs and canaries for being untouched.

Script mode (`python3 tests/galois_model.py --route`, a fresh process under a kernel trace): one NTT-domain automorphism over 17
limbs, then one rotation key product over 16 limbs, each checked (the route proof).
"""
import random

import numpy as np

import rns_support as rs

TRANSFORMED, ACCUMULATE, KEY_BROADCAST = 1, 2, 4


def bitrev(n):
    """bitrev_m(s) for every s < n = 2^m"""
    m = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(m):
        r |= ((np.arange(n, dtype=np.int64) >> b) & 1) << (m - 1 - b)
    return r


def ntt_source(n, g):
    """NTT domain: src[s] = bitrev(j), j = (g i + (g - 1) / 2) mod N, i = bitrev(s): out[s] = in[src[s]]"""
    rev = bitrev(n)
    j = (g * rev + (g - 1) // 2) % n
    return rev[j]


def coef_source(n, g):
    """coefficients: (src, neg) with u = g^-1 t mod 2N: out[t] = a[src[t]], negated where neg[t]"""
    u = (pow(g, -1, 2 * n) * np.arange(n, dtype=np.int64)) % (2 * n)
    return u % n, u >= n


def g_list(n, seed=0):
    """the issue's list of Galois elements, reduced mod 2N, in order and without repeats"""
    rng = random.Random(1000 * n + seed)
    raw = [1, 3, 5, 25, n - 1, n + 1, 2 * n - 1, pow(5, n // 4, 2 * n), rng.randrange(1, 2 * n, 2), rng.randrange(1, 2 * n, 2)]
    out = []
    for g in raw:
        g %= 2 * n
        if g % 2 and g not in out:
            out.append(g)
    return out


def rotation(n, steps):
    """5^steps mod 2N, negative steps the inverse power"""
    return pow(5, steps, 2 * n)


def _polys(a, n):
    return np.asarray(a, dtype=np.uint64).reshape(-1, n)


def ntt_model(a, n, g):
    """sigma_g on [batch][N] words in the NTT domain (bit-reversed storage): a permutation, any 64-bit words"""
    return _polys(a, n)[:, ntt_source(n, g)].reshape(-1)


def coef_model(a, n, g, q):
    """sigma_g on [batch][N] canonical coefficients mod q"""
    src, neg = coef_source(n, g)
    v = _polys(a, n)[:, src]
    return np.where(neg[None, :] & (v != 0), np.uint64(q) - v, v).reshape(-1)


def dot_model(orc, c, a_list, key_list, n, g, q, flags):
    """c (+)= sum_i sigma_g(a_i) (.) key_i in the NTT domain, canonical words; KEY_BROADCAST: every key is one polynomial"""
    acc = orc.dot([ntt_model(a, n, g) for a in a_list], key_list, q, N=n, bcast=bool(flags & KEY_BROADCAST))
    if flags & ACCUMULATE:
        acc = (acc + np.asarray(c, dtype=np.uint64)) % np.uint64(q)  # < 2^62: no wrap
    return acc


# ---------------------------------------------------------------- GPU case runners

def operand(orc, primes, n, batch, seed):
    """canonical random limbs ([batch][N] each) with the extremes of the range in the first slots"""
    limbs = [orc.fill_uniform(batch * n, q, seed * 1000 + l) for l, q in enumerate(primes)]
    for l, q in enumerate(primes):
        edge = [0, q - 1, (q - 1) // 2, (q + 1) // 2][:min(4, n)]
        limbs[l][:len(edge)] = edge
    return limbs


class Placed:
    """an operand uploaded in a layout among canaries"""

    def __init__(self, lib, limbs, n, batch, layout, bcast=False):
        self.nl, self.n, self.batch = len(limbs), n, 1 if bcast else batch
        if bcast:
            self.ls, self.ps, self.words = n, n, self.nl * n
        else:
            self.ls, self.ps, self.words = rs.layout_strides(layout, n, self.nl, batch)
        self.img = rs.place(limbs, n, self.batch, self.ls, self.ps, self.words)
        self.buf = lib.DeviceBuffer(self.words).upload(self.img)
        self.ptr = self.buf.ptr

    def download(self):
        """(limbs, whether every word outside the operand still holds what was uploaded)"""
        got = self.buf.download()
        limbs, used = rs.extract(got, self.nl, self.n, self.batch, self.ls, self.ps)
        return limbs, np.array_equal(got[~used], self.img[~used])

    def unchanged(self):
        return np.array_equal(self.buf.download(), self.img)

    def free(self):
        self.buf.free()


def _lay(layout, n, nl, batch):
    ls, ps, _ = rs.layout_strides(layout, n, nl, batch)
    return None if layout == "limb" else (ls, ps)


def run_galois(lib, orc, primes, roots, n, batch, g, flags, layout="limb", seed=1, plans=None, limbs=None):
    """one automorphism, every output word against the model; the input and the canaries untouched.  Returns the output limbs."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    if limbs is None:
        limbs = operand(orc, primes, n, batch, seed)
    src = Placed(lib, limbs, n, batch, layout)
    dst = Placed(lib, [np.full(batch * n, 0xDEAD, dtype=np.uint64) for _ in primes], n, batch, layout)
    try:
        lib.rns_galois(plans, dst.ptr, src.ptr, g, batch, flags, layout=_lay(layout, n, len(primes), batch))
        got, clean = dst.download()
        assert clean, "a word outside the output changed"
        assert src.unchanged(), "the input changed"
    finally:
        src.free(), dst.free()
        if own:
            for p in plans:
                p.destroy()
    for l, q in enumerate(primes):
        want = ntt_model(limbs[l], n, g) if flags & TRANSFORMED else coef_model(limbs[l], n, g, q)
        assert np.array_equal(got[l], want), "limb %d of %d differs from the model (N=%d, batch %d, g %d, flags %d, %s)" % (
            l, len(primes), n, batch, g, flags, layout)
    return got


def run_dot(lib, orc, primes, roots, n, batch, k, g, flags, layout="limb", seed=1, plans=None, extreme=False):
    """one rotation key product, every output word against the model; the operands and the canaries untouched.  extreme: every
    operand word (and c) is q - 1.  Returns the output limbs."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    bc = bool(flags & KEY_BROADCAST)

    def words(count, s):
        if extreme:
            return [np.full(count, q - 1, dtype=np.uint64) for q in primes]
        return [orc.fill_uniform(count, q, s * 1000 + l) for l, q in enumerate(primes)]

    a = [operand(orc, primes, n, batch, seed + 10 * i) if not extreme else words(batch * n, 0) for i in range(k)]
    key = [words(n if bc else batch * n, seed + 10 * i + 5) for i in range(k)]
    c0 = words(batch * n, seed + 7)
    pa = [Placed(lib, x, n, batch, layout) for x in a]
    pk = [Placed(lib, x, n, batch, layout, bcast=bc) for x in key]
    pc = Placed(lib, c0, n, batch, layout)
    try:
        lib.rns_galois_dot(plans, pc.ptr, [x.ptr for x in pa], [x.ptr for x in pk], g, batch, flags, layout=_lay(layout, n, len(primes), batch))
        got, clean = pc.download()
        assert clean, "a word outside the output changed"
        assert all(x.unchanged() for x in pa + pk), "an operand changed"
    finally:
        for x in pa + pk + [pc]:
            x.free()
        if own:
            for p in plans:
                p.destroy()
    for l, q in enumerate(primes):
        want = dot_model(orc, c0[l], [x[l] for x in a], [x[l] for x in key], n, g, q, flags)
        assert np.array_equal(got[l], want), "limb %d of %d differs from the model (N=%d, batch %d, k %d, g %d, flags %d, %s)" % (
            l, len(primes), n, batch, k, g, flags, layout)
    return got


def route(lib, orc):
    """2^12, 4 polynomials: an NTT-domain automorphism over 17 limbs (two launches), then a rotation key product of k = 3 over 16
    limbs (one launch)"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, [60] + [50] * 16)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    g = rotation(n, 3)
    run_galois(lib, orc, primes, roots, n, 4, g, TRANSFORMED, plans=plans, seed=17)
    run_dot(lib, orc, primes[:16], roots[:16], n, 4, 3, g, TRANSFORMED | KEY_BROADCAST, plans=plans[:16], seed=18)
    for p in plans:
        p.destroy()
    print("galois route: one automorphism over 17 limbs, one key product over 16 limbs")


def main():
    lib, orc = rs.load()
    route(lib, orc)


if __name__ == "__main__":
    main()
