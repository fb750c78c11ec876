"""Model of ntt_rns_mod_up_mul_batch -- c^ (+)= fwd(ModUp(digit)) (.) key^ on every limb of the extended basis -- for the tests, built
from what is there: keyswitch_model.mod_up(..., flags=0), then per limb Oracle().ctx(n, q, w).fwd, Oracle().pointwise and the
addition mod q (nothing of the kernels' arithmetic); the case runner of tests/test_gpu_modup_mul.py.

Script mode (`python3 tests/modup_mul_model.py`, a fresh process under a kernel trace): one checked call per modup_mul_kernel
instance (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W; <ArithF64,14,1> by the route call alone) and the route call: 2^14,
16 50-bit limbs and 2 60-bit limbs, digit (0, 2), NTT_OPT_MODUP_FUSED 1.
"""

import numpy as np

import keyswitch_model as km
import rns_support as rs

LAZY_IN, BROADCAST, ACCUMULATE = 1, 2, 4
SENTINEL = 0x5E47195E47195E47  # what d_ext's non-digit slots hold before the call


def model(orc, primes, roots, digit, key, acc, n, batch, first, count, flags):
    """digit: count arrays of batch * n canonical coefficients; key: one array per limb (n words with BROADCAST, else batch * n;
    words may be lazy with LAZY_IN); acc: one array per limb (used with ACCUMULATE).  Returns (c^ per limb, the limbs of d_ext as
    ntt_rns_mod_up_batch(flags = 0) leaves them)."""
    ext = [np.zeros(batch * n, dtype=np.uint64) for _ in primes]
    for i in range(count):
        ext[first + i] = np.asarray(digit[i], dtype=np.uint64)
    ext = km.mod_up(orc, primes, roots, ext, n, first, count, 0)
    out = []
    for l, (q, w) in enumerate(zip(primes, roots)):
        k = np.asarray(key[l], dtype=np.uint64) % np.uint64(q)
        if flags & BROADCAST:
            k = np.tile(k, batch)
        t = orc.pointwise(orc.ctx(n, q, w).fwd(ext[l]), k, q)
        out.append((np.asarray(acc[l], dtype=np.uint64) + t) % np.uint64(q) if flags & ACCUMULATE else t)  # < 2^62: no wrap
    return out, ext


def operands(orc, primes, n, batch, first, count, flags, seed, digit_max=False):
    """(digit, key, acc): random canonical words with the extremes keyswitch_model._operand plants; digit_max: every digit word
    b_i - 1 (the largest 128-bit sum); LAZY_IN: key words up to min(4q, 2^53) - 1"""
    coef = km._operand(orc, primes, None, n, batch, 0, seed)
    digit = [np.full(batch * n, primes[first + i] - 1, dtype=np.uint64) if digit_max else coef[first + i] for i in range(count)]
    kw = n if flags & BROADCAST else batch * n
    key, acc = [], []
    for l, q in enumerate(primes):
        top = min(4 * q, 1 << 53) if flags & LAZY_IN else q
        k = orc.fill_uniform(kw, top, seed * 1000 + 100 + l)
        k[:4] = [0, top - 1, (q - 1) // 2, (q + 1) // 2]
        a = orc.fill_uniform(batch * n, q, seed * 1000 + 200 + l)
        a[:4] = [q - 1, 0, (q + 1) // 2, (q - 1) // 2]
        key.append(k)
        acc.append(a)
    return digit, key, acc


def run(lib, orc, primes, roots, first, count, n, batch, flags, layout="limb", fused=None, seed=1, plans=None, digit_max=False,
        max_grid=None):
    """one call, every word of c^ compared with the model, the words outside the operands and the key unchanged.  Returns
    (c^ per limb, the limbs of d_ext after the call, the model's ModUp'd limbs)."""
    nl = len(primes)
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    digit, key, acc = operands(orc, primes, n, batch, first, count, flags, seed, digit_max)
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    ext_limbs = [digit[l - first] if first <= l < first + count else np.full(batch * n, SENTINEL, dtype=np.uint64) for l in range(nl)]
    ext_img = rs.place(ext_limbs, n, batch, ls, ps, words)
    c_img = rs.place(acc, n, batch, ls, ps, words)
    key_img = np.concatenate(key) if flags & BROADCAST else rs.place(key, n, batch, ls, ps, words)
    dext, dc, dk = lib.DeviceBuffer(words).upload(ext_img), lib.DeviceBuffer(words).upload(c_img), lib.DeviceBuffer(key_img.size).upload(key_img)
    try:
        if fused is not None:
            plans[0].set_option(lib.OPT_MODUP_FUSED, fused)
        if max_grid is not None:
            for p in plans:
                p.set_option(lib.OPT_MAX_GRID, max_grid)
        lib.rns_mod_up_mul(plans, dc.ptr, dext.ptr, first, count, dk.ptr, batch, flags, layout=None if layout == "limb" else (ls, ps))
        got_c, got_ext, got_key = dc.download(), dext.download(), dk.download()
    finally:
        dext.free(), dc.free(), dk.free()
        if own:
            for p in plans:
                p.destroy()
    want, up = model(orc, primes, roots, digit, key, acc, n, batch, first, count, flags)
    c, used = rs.extract(got_c, nl, n, batch, ls, ps)
    ext, _ = rs.extract(got_ext, nl, n, batch, ls, ps)
    for l in range(nl):
        assert np.array_equal(c[l], want[l]), "c^ limb %d of %d differs from the model (N=%d, batch %d, digit [%d, %d), flags %d, %s)" % (
            l, nl, n, batch, first, first + count, flags, layout)
    assert np.array_equal(got_c[~used], c_img[~used]), "a word outside c^ changed"
    assert np.array_equal(got_ext[~used], ext_img[~used]), "a word outside d_ext changed"
    assert np.array_equal(got_key, key_img), "the key changed"
    return c, ext, up


def untouched(ext, first, count):
    """the non-digit slots of d_ext that still hold the sentinel in every word"""
    return [l for l, e in enumerate(ext) if not first <= l < first + count and bool(np.all(e == np.uint64(SENTINEL)))]


def route(lib, orc):
    """2^14, 16 limbs of 50-bit primes (one run of the FP64 policy) and 2 of 60-bit primes, digit (0, 2), the fused kernel asked for:
    the FP64 run's slots of d_ext keep the sentinel"""
    n, first, count = 1 << 14, 0, 2
    primes, roots = rs.chain(lib, n, [50] * 16 + [60, 60])
    _, ext, _ = run(lib, orc, primes, roots, first, count, n, 2, BROADCAST | ACCUMULATE, fused=1, seed=17)
    assert untouched(ext, first, count)[:14] == list(range(2, 16)), "the FP64 run's slots of d_ext were written"
    print("modup_mul route: one call at 2^14 over 16 + 2 limbs")


def main():
    lib, orc = rs.load()
    driven = 0
    for pol, k, logn in rs.fused_launch_cases():
        if (pol, k, logn) == ("ArithF64", 1, 14):
            continue  # the route call's instance: launched exactly once in this process
        n = 1 << logn
        b = rs.CLASS_BITS[(pol, k)]
        primes, roots = rs.chain(lib, n, [b, b, b])
        run(lib, orc, primes, roots, 1, 2, n, 2, BROADCAST | ACCUMULATE, fused=1, seed=logn)
        driven += 1
    route(lib, orc)
    print("modup_mul launch proof: %d instances driven" % (driven + 1))


if __name__ == "__main__":
    main()
