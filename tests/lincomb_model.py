"""Model of the RNS linear combination (ntt_rns_lincomb_batch) for the tests: the definition of include/ntt_mi355x.h in Python integers
(limb_model: numpy object arrays, nothing of the kernel's arithmetic; src_g is galois_model.ntt_source), the same through the
oracle's modular product for the large shapes (limb_fast; tests/test_lincomb_cpu.py holds the two equal), and the case runner of
tests/test_gpu_lincomb.py, which places every operand in its layout among canaries and checks the output word for word and the
inputs and canaries for being untouched.

Script mode (`python3 tests/lincomb_model.py --route`, a fresh process under a kernel trace): one call over 16 limbs, then one over 17,
each behind the creation of its own plans (whose table kernels separate the two calls in the trace).
"""
import random

import numpy as np

import galois_model as gm
import rns_support as rs

ACCUMULATE, M_BROADCAST, LAZY_IN = 1, 2, 4


def _permuted(a, n, g):
    """a_i[p, src_g(s)] for [batch][N] words"""
    return np.asarray(a, dtype=np.uint64).reshape(-1, n)[:, gm.ntt_source(n, g)]


def limb_model(c, a_list, m_list, scalars, gs, bias, n, q, flags):
    """one limb, Python integers: c, a_i: [batch][N] words; m_list[i]: None or [batch][N] words ([N] with M_BROADCAST); scalars[i],
    bias: this limb's.  (c + bias + sum_i a_i[src_{g_i}(s)] * mu_i) mod q, c only with ACCUMULATE."""
    batch = np.asarray(a_list[0]).size // n
    acc = np.full((batch, n), int(bias), dtype=object)
    if flags & ACCUMULATE:
        acc = acc + np.asarray(c, dtype=np.uint64).reshape(batch, n).astype(object)
    for a, m, s, g in zip(a_list, m_list, scalars, gs):
        x = _permuted(a, n, g).astype(object)
        if m is None:
            acc = acc + x * int(s)
        else:
            mm = np.asarray(m, dtype=np.uint64).astype(object)
            acc = acc + x * (mm.reshape(1, n) if flags & M_BROADCAST else mm.reshape(batch, n))
    return (acc % int(q)).astype(np.uint64).reshape(-1)


def limb_fast(orc, c, a_list, m_list, scalars, gs, bias, n, q, flags):
    """limb_model through the oracle's modular product: every term reduced mod q, summed mod q (words below 2^62: no wrap)"""
    batch = np.asarray(a_list[0]).size // n
    Q = np.uint64(q)
    acc = np.full(batch * n, int(bias), dtype=np.uint64)
    if flags & ACCUMULATE:
        acc = (acc + np.asarray(c, dtype=np.uint64)) % Q
    for a, m, s, g in zip(a_list, m_list, scalars, gs):
        x = np.ascontiguousarray(_permuted(a, n, g).reshape(-1) % Q)
        if m is None:
            y = np.full(batch * n, int(s), dtype=np.uint64)
        else:
            mm = np.asarray(m, dtype=np.uint64)
            y = np.ascontiguousarray(np.tile(mm, batch) if flags & M_BROADCAST else mm)
        acc = (acc + orc.pointwise(x, y, q)) % Q
    return acc


def model(primes, c, a, m, scalars, gs, bias, n, flags, orc=None):
    """every limb: c[l], a[i][l], m[i] (None or [l]), scalars[i][l], bias[l]; orc: the large-shape route"""
    k = len(a)
    out = []
    for l, q in enumerate(primes):
        args = (c[l], [a[i][l] for i in range(k)], [None if m[i] is None else m[i][l] for i in range(k)], [scalars[i][l] for i in range(k)],
                gs, bias[l], n, q, flags)
        out.append(limb_fast(orc, *args) if orc is not None else limb_model(*args))
    return out


# ---------------------------------------------------------------- GPU case runner

def distinct_scalars(primes, k, seed):
    """scalars [k][limb] and bias [limb], every one different and below its prime, the extremes among them"""
    rng = random.Random(seed)
    s = [[rng.randrange(2, q) for q in primes] for _ in range(k)]
    s[0][0] = primes[0] - 1
    return s, [rng.randrange(1, q) for q in primes]


class Placed(gm.Placed):
    """galois_model.Placed, the layout also as (limb_stride, poly_stride, words) of the caller's own"""

    def __init__(self, lib, limbs, n, batch, layout, bcast=False):
        if bcast or not isinstance(layout, tuple):
            gm.Placed.__init__(self, lib, limbs, n, batch, "limb" if isinstance(layout, tuple) else layout, bcast)
            return
        self.nl, self.n, self.batch = len(limbs), n, batch
        self.ls, self.ps, self.words = layout
        self.img = rs.place(limbs, n, batch, self.ls, self.ps, self.words)
        self.buf = lib.DeviceBuffer(self.words).upload(self.img)
        self.ptr = self.buf.ptr


def _lay(layout, n, nl, batch):
    return layout[:2] if isinstance(layout, tuple) else gm._lay(layout, n, nl, batch)


def run_case(lib, orc, primes, roots, n, batch, gs, poly=(), flags=0, scalars="distinct", bias="distinct", layout="limb", seed=1, plans=None,
             fill=None, null_m=False, alias=None, big=None):
    """one call, every output word against the model; the inputs and the canaries untouched.  gs: one Galois element per term;
    poly: the terms with a polynomial multiplier; scalars / bias: "distinct", None (passed as NULL) or the values; fill: a function
    (q -> word) every operand word and c take; null_m: d_m itself NULL (no polynomial term); alias: ("a", i) or ("m", i) -- c is that
    operand.  Returns the output limbs."""
    k, nl = len(gs), len(primes)
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    bc = bool(flags & M_BROADCAST)
    lazy = bool(flags & LAZY_IN)

    def words(count, s, top=1):
        if fill:
            return [np.full(count, fill(q) if top == 1 else top * q - 1, dtype=np.uint64) for q in primes]
        return [orc.fill_uniform(count, top * q, s * 1000 + l) for l, q in enumerate(primes)]

    a = [words(batch * n, seed + 10 * i, 4 if lazy else 1) for i in range(k)]
    if not fill:
        for i in range(k):
            for l, q in enumerate(primes):
                edge = [0, q - 1, (4 * q - 1) if lazy else (q - 1) // 2, (q + 1) // 2][:min(4, n)]
                a[i][l][:len(edge)] = edge
    m = [words(n if bc else batch * n, seed + 10 * i + 5) if i in poly else None for i in range(k)]
    c0 = words(batch * n, seed + 7)
    dist_s, dist_b = distinct_scalars(primes, k, seed)
    s_arg = dist_s if scalars == "distinct" else scalars
    b_arg = dist_b if bias == "distinct" else bias
    s_eff = s_arg if s_arg is not None else [[1] * nl] * k
    b_eff = b_arg if b_arg is not None else [0] * nl
    pa = [Placed(lib, x, n, batch, layout) for x in a]
    pm = [None if x is None else Placed(lib, x, n, batch, layout, bcast=bc) for x in m]
    if alias:
        pc = (pa if alias[0] == "a" else pm)[alias[1]]
        c0 = (a if alias[0] == "a" else m)[alias[1]]
    else:
        pc = Placed(lib, c0, n, batch, layout)
    everything = pa + [x for x in pm if x is not None] + ([] if alias else [pc])
    try:
        lib.rns_lincomb(plans, pc.ptr, [x.ptr for x in pa], None if null_m else [None if x is None else x.ptr for x in pm], s_arg, list(gs), b_arg,
                        batch, flags, layout=_lay(layout, n, nl, batch))
        got, clean = pc.download()
        assert clean, "a word outside the output changed"
        assert all(x.unchanged() for x in everything if x is not pc), "an operand changed"
    finally:
        for x in everything:
            x.free()
        if own:
            for p in plans:
                p.destroy()
    if big is None:
        big = nl * batch * n * k > (1 << 17)
    want = model(primes, c0, a, m, s_eff, gs, b_eff, n, flags, orc if big else None)
    for l in range(nl):
        assert np.array_equal(got[l], want[l]), "limb %d of %d differs from the model (N=%d, batch %d, g %s, poly %s, flags %d, %s)" % (
            l, nl, n, batch, list(gs), list(poly), flags, layout)
    return got


def route(lib, orc):
    """2^10, 3 polynomials, k = 3 with one polynomial multiplier and three Galois elements: over 16 limbs, then over 17, each call
    with plans of its own"""
    n = 1 << 10
    for nlimbs in (16, 17):
        primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 1))
        run_case(lib, orc, primes, roots, n, 3, [1, 5, 2 * n - 1], poly=(1,), seed=17)
    print("lincomb route: one call over 16 limbs, one over 17")


def main():
    lib, orc = rs.load()
    route(lib, orc)


if __name__ == "__main__":
    main()
