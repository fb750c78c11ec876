"""Model of the RNS rescale (ntt_rns_rescale_batch) for the tests: the formula of include/ntt_mi355x.h in numpy, its products through
the oracle's pointwise product and its transforms through Oracle().ctx; a Python-integer CRT reference for small sizes; the case
runner of tests/test_gpu_rescale.py.  Prime chains, layouts and the instance list are in tests/rns_support.py.

Script mode (`python3 tests/rescale_model.py`, a fresh process under a kernel trace): one call per rescale kernel instance -- every
rescale_fwd_kernel (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W) and rescale_coef_kernel -- each checked against the
model (the launch proof); `--route`: one NTT-domain call at 2^14 over 17 FP64 limbs (the route proof).
"""
import sys

import numpy as np

import rns_support as rs

TRANSFORMED, FLOOR = 1, 2


def digits(t, qL, q, floor):
    """u_l = ((t + h) mod q_L) mod q_l - h_l (mod q_l); floor: t mod q_l (t canonical mod q_L, numpy uint64)"""
    t = np.asarray(t, dtype=np.uint64)
    if floor:
        return t % np.uint64(q)
    h = (qL - 1) // 2
    w = t + np.uint64(h)  # < 2^62: no wrap
    w = np.where(w >= np.uint64(qL), w - np.uint64(qL), w)
    return (w % np.uint64(q) + np.uint64(q - h % q)) % np.uint64(q)


def model(orc, primes, roots, limbs, n, flags):
    """limbs: L+1 arrays of batch * n canonical words ([batch][N] each) in the call's domain.  Returns (kept limbs after the call,
    the dropped limb's slot after the call)"""
    qL = primes[-1]
    floor = bool(flags & FLOOR)
    t = orc.ctx(n, qL, roots[-1]).inv(limbs[-1]) if flags & TRANSFORMED else np.asarray(limbs[-1], dtype=np.uint64)
    out = []
    for q, w, c in zip(primes[:-1], roots[:-1], limbs[:-1]):
        u = digits(t, qL, q, floor)
        if flags & TRANSFORMED:
            u = orc.ctx(n, q, w).fwd(u)
        d = (np.asarray(c, dtype=np.uint64) + np.uint64(q) - u) % np.uint64(q)
        s = pow(qL, q - 2, q)
        out.append(orc.pointwise(d, np.full(d.size, s, dtype=np.uint64), q))
    return out, t


def crt_rescale(primes, coef_limbs, floor):
    """the definition: x = CRT(coef_limbs) in [0, Q), y = round(x / q_L) (floor: floor) mod Q / q_L, as residues mod q_0 .. q_{L-1}
    (Python integers: small sizes only)"""
    Q = 1
    for q in primes:
        Q *= q
    qL = primes[-1]
    Qp = Q // qL
    basis = []
    for q in primes:
        m = Q // q
        basis.append(m * pow(m % q, q - 2, q))
    size = len(coef_limbs[0])
    out = [np.zeros(size, dtype=np.uint64) for _ in primes[:-1]]
    for i in range(size):
        x = sum(int(c[i]) * b for c, b in zip(coef_limbs, basis)) % Q
        y = (x // qL if floor else (x + (qL - 1) // 2) // qL) % Qp
        for l, q in enumerate(primes[:-1]):
            out[l][i] = y % q
    return out


def residues(x, primes):
    """the RNS words of integers x (a list of Python ints) as [limb] arrays"""
    return [np.array([v % q for v in x], dtype=np.uint64) for q in primes]


def run_case(lib, orc, primes, roots, n, batch, flags, layout="limb", fused=None, seed=1, plans=None, crt=False):
    """one call on random canonical operands, checked word for word against the model (crt: also against the CRT definition),
    canaries and the dropped-limb contract included.  Returns the kept limbs after the call."""
    nl = len(primes)
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    if fused is not None:
        plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
    coef = [orc.fill_uniform(batch * n, q, seed * 1000 + l) for l, q in enumerate(primes)]
    if batch and n >= 4:  # the extremes of the canonical range
        for l, q in enumerate(primes):
            rs.edge_fill(coef[l], q)
    limbs = [orc.ctx(n, q, w).fwd(c) for q, w, c in zip(primes, roots, coef)] if flags & TRANSFORMED else coef
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    img = rs.place(limbs, n, batch, ls, ps, words)
    buf = lib.DeviceBuffer(words).upload(img)
    lib.rns_rescale(plans, buf.ptr, batch, flags, layout=None if layout == "limb" else (ls, ps))
    got_img = buf.download()
    buf.free()
    got, used = rs.extract(got_img, nl, n, batch, ls, ps)
    assert np.array_equal(got_img[~used], img[~used]), "a word outside the operand changed"
    want, t = model(orc, primes, roots, limbs, n, flags)
    for l in range(nl - 1):
        assert np.array_equal(got[l], want[l]), "limb %d of %d differs from the model (N=%d, batch %d, flags %d, %s)" % (
            l, nl - 1, n, batch, flags, layout)
    assert np.array_equal(got[-1], t if flags & TRANSFORMED else limbs[-1]), "the dropped limb's slot"
    if crt:
        ref = crt_rescale(primes, coef, bool(flags & FLOOR))
        for l, (q, w) in enumerate(zip(primes[:-1], roots[:-1])):
            c = orc.ctx(n, q, w).inv(got[l]) if flags & TRANSFORMED else got[l]
            assert np.array_equal(c, ref[l]), "limb %d differs from round/floor(x / q_L) over the CRT" % l
    if own:
        for p in plans:
            p.destroy()
    return got


def route(lib, orc):
    """2^14, 17 limbs of 50-bit primes (16 kept: one run of the FP64 policy), NTT domain, 8 polynomials: the route proof's call"""
    n = 1 << 14
    primes, roots = rs.chain(lib, n, [50] * 17)
    run_case(lib, orc, primes, roots, n, 8, TRANSFORMED, seed=17)
    print("rescale route: one call at 2^14 over 17 limbs")


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        n = 1 << logn
        primes, roots = rs.chain(lib, n, [rs.CLASS_BITS[(pol, k)]] * 3)
        run_case(lib, orc, primes, roots, n, 2, TRANSFORMED, seed=logn)
    primes, roots = rs.chain(lib, 1 << 10, [50, 50, 50])
    run_case(lib, orc, primes, roots, 1 << 10, 2, 0)
    print("rescale launch proof: %d instances driven" % (len(rs.fused_launch_cases()) + 1))


if __name__ == "__main__":
    main()
