"""Model of the first and the last step of a homomorphic multiplication on NTT-domain ciphertexts (ntt_rns_tensor_batch,
ntt_rns_mod_down_add_batch) for the tests: the formulas of include/ntt_mi355x.h in numpy, the modular products through the oracle's
pointwise product, ModDown through tests/keyswitch_model.py (nothing of the kernels' arithmetic); the case runners of
tests/test_gpu_ct_mul.py; the model of examples/rns_ciphertext_mul.c.

Script mode (`python3 tests/ct_mul_model.py`, a fresh process under a kernel trace): one checked call per new kernel instance --
every ksfold_fwd_kernel (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W), tensor_kernel and ct_fold_kernel (the launch
proof); `--route`: one fused NTT-domain call at 2^14 over 16 50-bit Q limbs and 2 60-bit P limbs (the route proof).
"""
import sys

import numpy as np

import keyswitch_model as km
import rescale_model as rm
import rns_support as rs

TRANSFORMED, FLOOR, ACCUMULATE = 1, 2, 4
LAZY_IN = 1


def tensor(orc, primes, a0, a1, b0, b1):
    """(c0, c1, c2) per limb: a0 b0, a0 b1 + a1 b0, a1 b1 mod q_l, canonical; the inputs are lists of per-limb arrays with words
    anywhere below 2^63 (reduced first: the product is a function of the residues)"""
    c0, c1, c2 = [], [], []
    for q, x0, x1, y0, y1 in zip(primes, a0, a1, b0, b1):
        x0, x1, y0, y1 = (rs.u64(v) % np.uint64(q) for v in (x0, x1, y0, y1))
        c0.append(orc.pointwise(x0, y0, q))
        c1.append((orc.pointwise(x0, y1, q) + orc.pointwise(x1, y0, q)) % np.uint64(q))  # < 2^62: no wrap
        c2.append(orc.pointwise(x1, y1, q))
    return c0, c1, c2


def mod_down_add(orc, primes, roots, np_, c, a, n, flags):
    """keyswitch_model.mod_down of the accumulator a (over Q u P), then c_l = r_l or, with ACCUMULATE, (c_l + r_l) mod q_l.
    Returns (the ciphertext's limbs after the call, the P limbs' slots of a after the call)"""
    r, t = km.mod_down(orc, primes, roots, np_, a, n, flags & (TRANSFORMED | FLOOR))
    if flags & ACCUMULATE:
        r = [(rs.u64(cl) + rl) % np.uint64(q) for cl, rl, q in zip(c, r, primes)]
    return r, t


# ---------------------------------------------------------------- GPU case runners

class _Image:
    """an operand on the device in a layout with canaries around it"""

    def __init__(self, lib, limbs, n, batch, layout):
        self.n, self.batch, self.nl = n, batch, len(limbs)
        if isinstance(layout, tuple):
            self.ls, self.ps, self.words = layout
        else:
            self.ls, self.ps, self.words = rs.layout_strides(layout, n, self.nl, batch)
        self.img = rs.place(limbs, n, batch, self.ls, self.ps, self.words)
        self.buf = lib.DeviceBuffer(self.words).upload(self.img)

    @property
    def ptr(self):
        return self.buf.ptr

    def limbs(self):
        """the limbs now on the device; asserts that no word outside the operand changed"""
        got = self.buf.download()
        out, used = rs.extract(got, self.nl, self.n, self.batch, self.ls, self.ps)
        assert np.array_equal(got[~used], self.img[~used]), "a word outside the operand changed"
        return out

    def free(self):
        self.buf.free()


def tensor_inputs(orc, primes, n, batch, seed, fill=None, lazy_limbs=()):
    """four operands: random canonical words with the extremes in front; fill = "zero" / "max": every word 0 / q - 1; limbs in
    lazy_limbs hold 4q - 1 everywhere (NTT_MUL_LAZY_IN's largest word)"""
    ops = []
    for j in range(4):
        limbs = []
        for l, q in enumerate(primes):
            if l in lazy_limbs:
                v = np.full(batch * n, 4 * q - 1, dtype=np.uint64)
            elif fill == "zero":
                v = np.zeros(batch * n, dtype=np.uint64)
            elif fill == "max":
                v = np.full(batch * n, q - 1, dtype=np.uint64)
            else:
                v = orc.fill_uniform(batch * n, q, seed * 1000 + 100 * j + l)
                v[:2] = [q - 1, 0] if j % 2 else [0, q - 1]
            limbs.append(v)
        ops.append(limbs)
    return ops


def run_tensor(lib, orc, primes, n, batch, ops, flags=0, layout="limb", mode="general", plans=None, roots=None):
    """one tensor call, every output word against the model, canaries and the inputs' contract included.  mode: "general" (seven
    buffers), "square" (b0 = a0 and b1 = a1 by pointer), "inplace" (c0 = a0, c1 = a1 by pointer).  Returns (c0, c1, c2)."""
    own = plans is None
    if own:
        roots = roots or [lib.min_root(q, n) for q in primes]
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    a0, a1, b0, b1 = ops
    if mode == "square":
        b0, b1 = a0, a1
    ins = [_Image(lib, v, n, batch, layout) for v in ((a0, a1) if mode == "square" else (a0, a1, b0, b1))]
    if mode == "square":
        ins += ins
    blank = [np.full(batch * n, 0xDEAD, dtype=np.uint64) for _ in primes]
    outs = [ins[0], ins[1]] if mode == "inplace" else [_Image(lib, blank, n, batch, layout) for _ in range(2)]
    outs.append(_Image(lib, blank, n, batch, layout))
    lay = None if layout == "limb" else (ins[0].ls, ins[0].ps)
    try:
        lib.rns_tensor(plans, outs[0].ptr, outs[1].ptr, outs[2].ptr, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, batch, flags, layout=lay)
        got = [o.limbs() for o in outs]
        kept = [i.limbs() for i in ins[2:]] if mode == "inplace" else [i.limbs() for i in ins]
    finally:
        for o in {id(x): x for x in ins + outs}.values():
            o.free()
        if own:
            for p in plans:
                p.destroy()
    want = tensor(orc, primes, a0, a1, b0, b1)
    for j in range(3):
        for l in range(len(primes)):
            assert np.array_equal(got[j][l], want[j][l]), "c%d limb %d of %d differs from the model (N=%d, batch %d, flags %d, %s, %s)" % (
                j, l, len(primes), n, batch, flags, layout, mode)
    for i, (k, v) in enumerate(zip(kept, (b0, b1) if mode == "inplace" else (a0, a1, b0, b1))):
        for l in range(len(primes)):
            assert np.array_equal(k[l], v[l]), "input %d limb %d changed" % (i, l)
    return got


def run_down_add(lib, orc, primes, roots, np_, n, batch, flags, c_layout="limb", a_layout="limb", fused=None, rescale_fused=None, seed=1,
                 plans=None, a_untouched=None, cross_check=True):
    """one ModDown-add on random canonical operands: every word of the ciphertext against the model and against rns_mod_down on a copy
    plus a numpy addition; the accumulator's P slots; its Q limbs unchanged where a_untouched; canaries.  Returns the ciphertext's limbs."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    nq = len(primes) - np_
    dom = flags & TRANSFORMED
    a = km._operand(orc, primes, roots, n, batch, dom, seed)
    c = km._operand(orc, primes[:nq], roots[:nq], n, batch, dom, seed + 50)
    ia, ic, ib = _Image(lib, a, n, batch, a_layout), _Image(lib, c, n, batch, c_layout), None
    lay = None if (c_layout, a_layout) == ("limb", "limb") else (ic.ls, ic.ps, ia.ls, ia.ps)
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_MODDOWN_ADD_FUSED, fused)
        if rescale_fused is not None:
            plans[0].set_option(lib.OPT_RESCALE_FUSED, rescale_fused)
        lib.rns_mod_down_add(plans, np_, ic.ptr, ia.ptr, batch, flags, layout=lay)
        got, after = ic.limbs(), ia.limbs()
        if cross_check:
            ib = _Image(lib, a, n, batch, "limb")
            lib.rns_mod_down(plans, np_, ib.ptr, batch, flags & (TRANSFORMED | FLOOR))
            r = ib.limbs()[:nq]
    finally:
        if fused is not None:
            plans[0].set_option(lib.OPT_MODDOWN_ADD_FUSED, -1)
        if rescale_fused is not None:
            plans[0].set_option(lib.OPT_RESCALE_FUSED, 1)
        for o in (ia, ic, ib):
            if o is not None:
                o.free()
        if own:
            for p in plans:
                p.destroy()
    want, t = mod_down_add(orc, primes, roots, np_, c, a, n, flags)
    what = "(N=%d, batch %d, nq %d, np %d, flags %d, c %s, a %s)" % (n, batch, nq, np_, flags, c_layout, a_layout)
    for l in range(nq):
        assert np.array_equal(got[l], want[l]), "limb %d differs from the model %s" % (l, what)
        if cross_check:
            two = (c[l] + r[l]) % np.uint64(primes[l]) if flags & ACCUMULATE else r[l]
            assert np.array_equal(got[l], two), "limb %d differs from rns_mod_down plus the addition %s" % (l, what)
    for j in range(np_):
        assert np.array_equal(after[nq + j], t[j] if dom else a[nq + j]), "P slot %d %s" % (j, what)
    if a_untouched:
        for l in range(nq):
            assert np.array_equal(after[l], a[l]), "the accumulator's Q limb %d was written %s" % (l, what)
    return got


# ---------------------------------------------------------------- the example

def example_primes(lib, n):
    """examples/rns_ciphertext_mul.c: Q = one 60-bit and seven 50-bit primes, P = two 60-bit primes"""
    primes = [lib.find_prime(60, n, 0)] + [lib.find_prime(50, n, k) for k in range(7)] + [lib.find_prime(60, n, k) for k in (1, 2)]
    return primes, [lib.min_root(q, n) for q in primes]


def example_model(lib, orc):
    """{(component, limb): checksum} of examples/rns_ciphertext_mul.c: tensor, inverse of d2, four digits of two limbs through ModUp
    and both key products, ModDown into (d0, d1), rescale by the last Q prime"""
    n, nq, np_, alpha = 1 << 13, 8, 2, 2
    primes, roots = example_primes(lib, n)
    ct = [[orc.fill_uniform(n, q, 100 + 16 * j + l) for l, q in enumerate(primes[:nq])] for j in range(4)]  # a0, a1, b0, b1
    d0, d1, d2 = tensor(orc, primes[:nq], *ct)
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
        c, _ = mod_down_add(orc, primes, roots, np_, d, acc[j], n, TRANSFORMED | ACCUMULATE)
        kept, _ = rm.model(orc, primes[:nq], roots[:nq], c, n, TRANSFORMED)
        for l in range(nq - 1):
            out[(j, l)] = orc.checksum(kept[l])
    return out


def route(lib, orc):
    """2^14, 16 Q limbs of 50-bit primes (one run of the FP64 policy) and 2 P limbs of 60-bit primes, NTT domain, accumulating, batch 2,
    the fused route forced"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, [50] * 16 + [60, 60])
    run_down_add(lib, orc, primes, roots, 2, n, 2, TRANSFORMED | ACCUMULATE, fused=1, seed=17, a_untouched=True, cross_check=False)
    print("ksfold route: one call at 2^14 over 16 + 2 limbs")


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        n = 1 << logn
        b = rs.CLASS_BITS[(pol, k)]
        primes, roots = rs.chain(lib, n, [b, b, 60, 60])
        run_down_add(lib, orc, primes, roots, 2, n, 2, TRANSFORMED | (ACCUMULATE if logn % 2 else 0), fused=1, seed=logn, a_untouched=True,
                     cross_check=False)
    primes, roots = rs.chain(lib, 1 << 10, [50, 50, 50, 60])
    run_down_add(lib, orc, primes, roots, 1, 1 << 10, 2, ACCUMULATE, cross_check=False)  # coefficients: ct_fold_kernel
    run_tensor(lib, orc, primes, 1 << 10, 2, tensor_inputs(orc, primes, 1 << 10, 2, 3))
    print("ct_mul launch proof: %d instances driven" % (len(rs.fused_launch_cases()) + 2))


if __name__ == "__main__":
    main()
