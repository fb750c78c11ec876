"""Model of the RNS base conversions of hybrid key switching (ntt_rns_mod_up_batch, ntt_rns_mod_down_batch) for the tests: the
formulas of include/ntt_mi355x.h in numpy, their modular products through the oracle's pointwise product and their transforms
through Oracle().ctx (nothing of the kernels' arithmetic); Python-integer CRT references for small sizes; the case runners of
tests/test_gpu_keyswitch.py.

Script mode (`python3 tests/keyswitch_model.py`, a fresh process under a kernel trace): one checked call per new kernel instance --
every moddown_fwd_kernel (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W), moddown_coef_kernel and bconv_kernel (the
launch proof); `--route`: one NTT-domain ModDown at 2^14 over 16 50-bit Q limbs and 2 60-bit P limbs (the route proof).
"""
import sys

import numpy as np

import rns_support as rs

TRANSFORMED, FLOOR = 1, 2


def prod(xs):
    r = 1
    for x in xs:
        r *= x
    return r


def bconv(orc, basis, digits, q, offsets=None):
    """FastBConv_{B->q}: ( sum_i [ (x_i + o_i) * b^_i^-1 ]_{b_i} * b^_i ) mod q, for digits x_i canonical mod b_i (numpy uint64),
    offsets o_i added mod b_i first (ModDown's [h]_{p_i}).  The products through orc.pointwise."""
    B = prod(basis)
    acc = np.zeros(len(digits[0]), dtype=np.uint64)
    for i, (b, x) in enumerate(zip(basis, digits)):
        w = rs.u64(x)
        if offsets:
            w = (w + np.uint64(offsets[i])) % np.uint64(b)  # < 2^62: no wrap
        hat = B // b
        z = orc.pointwise(w, rs.full(w.size, pow(hat % b, -1, b)), b)
        term = orc.pointwise(z % np.uint64(q), rs.full(w.size, hat % q), q)
        acc = (acc + term) % np.uint64(q)  # < 2^62: no wrap
    return acc


def mod_up(orc, primes, roots, limbs, n, first, count, flags):
    """limbs: the operand's arrays (batch * n words each) in the call's domain.  Returns every limb after the call."""
    digit = list(range(first, first + count))
    basis = [primes[i] for i in digit]
    coef = [orc.ctx(n, primes[i], roots[i]).inv(limbs[i]) if flags & TRANSFORMED else rs.u64(limbs[i]) for i in digit]
    out = []
    for l, (q, w) in enumerate(zip(primes, roots)):
        if first <= l < first + count:
            out.append(rs.u64(limbs[l]))
            continue
        v = bconv(orc, basis, coef, q)
        out.append(orc.ctx(n, q, w).fwd(v) if flags & TRANSFORMED else v)
    return out


def mod_down_digits(orc, pr, t, q, floor):
    """u = FastBConv_{P->q}([t + h]_P) - [h]_q (mod q), t the P limbs' coefficients"""
    P = prod(pr)
    h = 0 if floor else (P - 1) // 2
    conv = bconv(orc, pr, t, q, offsets=None if floor else [h % p for p in pr])
    return (conv + np.uint64(q - h % q)) % np.uint64(q)


def mod_down(orc, primes, roots, np_, limbs, n, flags):
    """the last np_ primes are P.  Returns (Q limbs after the call, the P limbs' slots after the call)"""
    nq = len(primes) - np_
    pr = primes[nq:]
    floor = bool(flags & FLOOR)
    t = [orc.ctx(n, p, w).inv(c) if flags & TRANSFORMED else rs.u64(c) for p, w, c in zip(pr, roots[nq:], limbs[nq:])]
    P = prod(pr)
    out = []
    for q, w, c in zip(primes[:nq], roots[:nq], limbs[:nq]):
        u = mod_down_digits(orc, pr, t, q, floor)
        if flags & TRANSFORMED:
            u = orc.ctx(n, q, w).fwd(u)
        d = (rs.u64(c) + np.uint64(q) - u) % np.uint64(q)
        out.append(orc.pointwise(d, rs.full(d.size, pow(P % q, -1, q)), q))
    return out, t


# ---------------------------------------------------------------- CRT references (Python integers, small sizes)

def crt(residues, primes):
    """the integers in [0, prod) with the given residues (one list per prime)"""
    M = prod(primes)
    basis = [(M // q) * pow((M // q) % q, -1, q) for q in primes]
    return [sum(int(r[i]) * b for r, b in zip(residues, basis)) % M for i in range(len(residues[0]))]


def fastbconv_int(basis, xs, offsets=None):
    """the integer sum of FastBConv (before the reduction mod the target): sum_i [(x_i + o_i) b^_i^-1]_{b_i} b^_i"""
    B = prod(basis)
    out = []
    for k in range(len(xs[0])):
        s = 0
        for i, b in enumerate(basis):
            w = (int(xs[i][k]) + (offsets[i] if offsets else 0)) % b
            s += (w * pow((B // b) % b, -1, b) % b) * (B // b)
        out.append(s)
    return out


def residues(x, primes):
    return [np.array([v % q for v in x], dtype=np.uint64) for q in primes]


# (limb bit sizes, first, count) of the ModUp digits the CPU tests of the key-switch models use: at the start, in the middle, at the
# end, one limb, sixteen limbs
UP_CHAINS = [([50, 50, 50, 50, 60, 60], 0, 2), ([60, 50, 50, 50, 50, 60, 60], 1, 3), ([50] * 6 + [60, 60], 6, 2), ([30, 52, 50, 60], 1, 1),
             ([50] * 18, 1, 16)]


# ---------------------------------------------------------------- GPU case runners

def _operand(orc, primes, roots, n, batch, flags, seed):
    coef = [orc.fill_uniform(batch * n, q, seed * 1000 + l) for l, q in enumerate(primes)]
    if batch and n >= 4:  # the extremes of the canonical range
        for l, q in enumerate(primes):
            rs.edge_fill(coef[l], q)
    return [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & TRANSFORMED else coef


def _call(lib, fn, primes, n, batch, limbs, layout):
    nl = len(primes)
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    img = rs.place(limbs, n, batch, ls, ps, words)
    buf = lib.DeviceBuffer(words).upload(img)
    try:
        fn(buf.ptr, None if layout == "limb" else (ls, ps))
        got_img = buf.download()
    finally:
        buf.free()
    got, used = rs.extract(got_img, nl, n, batch, ls, ps)
    assert np.array_equal(got_img[~used], img[~used]), "a word outside the operand changed"
    return got


def run_down(lib, orc, primes, roots, np_, n, batch, flags, layout="limb", fused=None, seed=1, plans=None):
    """one ModDown on random canonical operands, every word checked against the model (the P slots included).  Returns the Q
    limbs after the call."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
        limbs = _operand(orc, primes, roots, n, batch, flags, seed)
        got = _call(lib, lambda ptr, lay: lib.rns_mod_down(plans, np_, ptr, batch, flags, layout=lay), primes, n, batch, limbs, layout)
    finally:
        if own:
            for p in plans:
                p.destroy()
    want, t = mod_down(orc, primes, roots, np_, limbs, n, flags)
    nq = len(primes) - np_
    for l in range(nq):
        assert np.array_equal(got[l], want[l]), "Q limb %d of %d differs from the model (N=%d, batch %d, np %d, flags %d, %s)" % (
            l, nq, n, batch, np_, flags, layout)
    for j in range(np_):
        assert np.array_equal(got[nq + j], t[j] if flags & TRANSFORMED else limbs[nq + j]), "P slot %d" % j
    return got[:nq]


def run_up(lib, orc, primes, roots, first, count, n, batch, flags, layout="limb", seed=1, plans=None):
    """one ModUp on random canonical operands, every word checked against the model.  Returns the limbs after the call."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    try:
        limbs = _operand(orc, primes, roots, n, batch, flags, seed)
        got = _call(lib, lambda ptr, lay: lib.rns_mod_up(plans, ptr, first, count, batch, flags, layout=lay), primes, n, batch, limbs,
                    layout)
    finally:
        if own:
            for p in plans:
                p.destroy()
    want = mod_up(orc, primes, roots, limbs, n, first, count, flags)
    for l in range(len(primes)):
        assert np.array_equal(got[l], want[l]), "limb %d of %d differs from the model (N=%d, batch %d, digit [%d, %d), flags %d, %s)" % (
            l, len(primes), n, batch, first, first + count, flags, layout)
    return got


def route(lib, orc):
    """2^14, 16 Q limbs of 50-bit primes (one run of the FP64 policy) and 2 P limbs of 60-bit primes, NTT domain, 4 polynomials"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, [50] * 16 + [60, 60])
    run_down(lib, orc, primes, roots, 2, n, 4, TRANSFORMED, seed=17)
    print("moddown route: one call at 2^14 over 16 + 2 limbs")


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        n = 1 << logn
        b = rs.CLASS_BITS[(pol, k)]
        primes, roots = rs.chain(lib, n, [b, b, 60, 60])
        run_down(lib, orc, primes, roots, 2, n, 2, TRANSFORMED, seed=logn)
    primes, roots = rs.chain(lib, 1 << 10, [50, 50, 50, 60])
    run_down(lib, orc, primes, roots, 1, 1 << 10, 2, 0)
    run_up(lib, orc, primes, roots, 1, 2, 1 << 10, 2, 0)
    print("keyswitch launch proof: %d instances driven" % (len(rs.fused_launch_cases()) + 2))


if __name__ == "__main__":
    main()
