"""Model of the pair key products -- ntt_rns_fwd_mul_pair_batch, ntt_rns_mod_up_mul_pair_batch, ntt_rns_galois_dot_pair_batch -- for the
tests, built from what is there: modup_mul_model.model (keyswitch_model.mod_up, Oracle().ctx(n, q, w).fwd, Oracle().pointwise) and
galois_model.dot_model, applied ONCE PER COMPONENT with that component's key and accumulator (nothing of the kernels' arithmetic);
the case runners of tests/test_gpu_key_pair.py.  key0 and key1 (and the two accumulators) are drawn from different seeds: a swapped
or duplicated component cannot pass.

Script mode (`python3 tests/key_pair_model.py`, a fresh process under a kernel trace): one checked call per modup_mul2_kernel
instance (N = 2^6..2^14 x ArithF64 classes 0, 1, 18 and ArithF64W; <ArithF64,14,1> by the route call alone) and the route call: 2^14,
16 50-bit limbs and 2 60-bit limbs, digit (0, 2), NTT_OPT_PAIR_FUSED 1.
"""

import numpy as np

import galois_model as gm
import modup_mul_model as mm
import rns_support as rs

LAZY_IN, BROADCAST, ACCUMULATE = mm.LAZY_IN, mm.BROADCAST, mm.ACCUMULATE
SENTINEL = mm.SENTINEL
KEY1_SEED = 7919  # added to the seed of component 1's key and accumulator


def model(orc, primes, roots, digit, keys, accs, n, batch, first, count, flags):
    """mod_up_mul_pair: ([c0^ per limb, c1^ per limb], ModUp's limbs of d_ext) -- modup_mul_model.model once per component"""
    outs, ext = [], None
    for j in range(2):
        o, ext = mm.model(orc, primes, roots, digit, keys[j], accs[j], n, batch, first, count, flags)
        outs.append(o)
    return outs, ext


def fwd_model(orc, primes, roots, a, keys, accs, n, batch, flags):
    """fwd_mul_pair: [c0^ per limb, c1^ per limb]; per component and limb fwd(a_l) (.) key_l (+ acc_l) as modup_mul_model.model forms
    it from its extended operand.  Also returns fwd(a) per limb (what the composition leaves in d_a)."""
    outs = []
    fa = [orc.ctx(n, q, w).fwd(np.asarray(a[l], dtype=np.uint64)) for l, (q, w) in enumerate(zip(primes, roots))]
    for j in range(2):
        out = []
        for l, q in enumerate(primes):
            k = np.asarray(keys[j][l], dtype=np.uint64) % np.uint64(q)
            if flags & BROADCAST:
                k = np.tile(k, batch)
            t = orc.pointwise(fa[l], k, q)
            out.append((np.asarray(accs[j][l], dtype=np.uint64) + t) % np.uint64(q) if flags & ACCUMULATE else t)  # < 2^62: no wrap
        outs.append(out)
    return outs, fa


def operands(orc, primes, n, batch, first, count, flags, seed, digit_max=False):
    """(digit, [key0, key1], [acc0, acc1]): modup_mul_model.operands twice, the second component from another seed"""
    digit, k0, a0 = mm.operands(orc, primes, n, batch, first, count, flags, seed, digit_max)
    _, k1, a1 = mm.operands(orc, primes, n, batch, first, count, flags, seed + KEY1_SEED, digit_max)
    for l in range(len(primes)):
        assert not np.array_equal(k0[l], k1[l])
    return digit, [k0, k1], [a0, a1]


def _options(lib, plans, fused, max_grid):
    if fused is not None:
        plans[0].set_option(lib.OPT_PAIR_FUSED, fused)
    if max_grid is not None:
        for p in plans:
            p.set_option(lib.OPT_MAX_GRID, max_grid)


def _check_pair(got_c, c_imgs, want, nl, n, batch, ls, ps, what):
    cs = []
    for j in range(2):
        c, used = rs.extract(got_c[j], nl, n, batch, ls, ps)
        for l in range(nl):
            assert np.array_equal(c[l], want[j][l]), "c%d^ limb %d of %d differs from the model (%s)" % (j, l, nl, what)
        assert np.array_equal(got_c[j][~used], c_imgs[j][~used]), "a word outside c%d^ changed" % j
        cs.append(c)
    return cs


def run(lib, orc, primes, roots, first, count, n, batch, flags, layout="limb", fused=None, seed=1, plans=None, digit_max=False,
        max_grid=None, single=False):
    """one ntt_rns_mod_up_mul_pair_batch call, every word of c0^ and c1^ compared with the model, the words outside the operands and
    both keys unchanged.  single: the same inputs also through two ntt_rns_mod_up_mul_batch calls (NTT_OPT_MODUP_FUSED as it stands),
    outputs compared word for word.  Returns ([c0^, c1^] per limb, the limbs of d_ext after the call, the model's ModUp'd limbs)."""
    nl = len(primes)
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    digit, keys, accs = operands(orc, primes, n, batch, first, count, flags, seed, digit_max)
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    lay = None if layout == "limb" else (ls, ps)
    ext_limbs = [digit[l - first] if first <= l < first + count else np.full(batch * n, SENTINEL, dtype=np.uint64) for l in range(nl)]
    ext_img = rs.place(ext_limbs, n, batch, ls, ps, words)
    c_imgs = [rs.place(accs[j], n, batch, ls, ps, words) for j in range(2)]
    key_imgs = [np.concatenate(keys[j]) if flags & BROADCAST else rs.place(keys[j], n, batch, ls, ps, words) for j in range(2)]
    dext = lib.DeviceBuffer(words).upload(ext_img)
    dc = [lib.DeviceBuffer(words).upload(c_imgs[j]) for j in range(2)]
    dk = [lib.DeviceBuffer(key_imgs[j].size).upload(key_imgs[j]) for j in range(2)]
    try:
        _options(lib, plans, fused, max_grid)
        lib.rns_mod_up_mul_pair(plans, dc[0].ptr, dc[1].ptr, dext.ptr, first, count, dk[0].ptr, dk[1].ptr, batch, flags, layout=lay)
        got_c, got_ext, got_key = [d.download() for d in dc], dext.download(), [d.download() for d in dk]
        if single:
            for j in range(2):
                dext.upload(ext_img), dc[j].upload(c_imgs[j])
                lib.rns_mod_up_mul(plans, dc[j].ptr, dext.ptr, first, count, dk[j].ptr, batch, flags, layout=lay)
                assert np.array_equal(dc[j].download(), got_c[j]), "c%d^ differs from the single call's" % j
    finally:
        dext.free()
        for d in dc + dk:
            d.free()
        if own:
            for p in plans:
                p.destroy()
    want, up = model(orc, primes, roots, digit, keys, accs, n, batch, first, count, flags)
    what = "N=%d, batch %d, digit [%d, %d), flags %d, %s" % (n, batch, first, first + count, flags, layout)
    cs = _check_pair(got_c, c_imgs, want, nl, n, batch, ls, ps, what)
    ext, used = rs.extract(got_ext, nl, n, batch, ls, ps)
    assert np.array_equal(got_ext[~used], ext_img[~used]), "a word outside d_ext changed"
    for j in range(2):
        assert np.array_equal(got_key[j], key_imgs[j]), "key%d changed" % j
    return cs, ext, up


def run_fwd(lib, orc, primes, roots, n, batch, flags, layout="limb", fused=None, seed=1, plans=None, max_grid=None, single=False):
    """one ntt_rns_fwd_mul_pair_batch call, every word of c0^ and c1^ compared with the model; the canaries and both keys unchanged.
    Returns ([c0^, c1^] per limb, the limbs of d_a after the call, the operand as uploaded, fwd(a) per limb)."""
    nl = len(primes)
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    a, keys, accs = operands(orc, primes, n, batch, 0, nl, flags, seed)
    ls, ps, words = rs.layout_strides(layout, n, nl, batch)
    lay = None if layout == "limb" else (ls, ps)
    a_img = rs.place(a, n, batch, ls, ps, words)
    c_imgs = [rs.place(accs[j], n, batch, ls, ps, words) for j in range(2)]
    key_imgs = [np.concatenate(keys[j]) if flags & BROADCAST else rs.place(keys[j], n, batch, ls, ps, words) for j in range(2)]
    da = lib.DeviceBuffer(words).upload(a_img)
    dc = [lib.DeviceBuffer(words).upload(c_imgs[j]) for j in range(2)]
    dk = [lib.DeviceBuffer(key_imgs[j].size).upload(key_imgs[j]) for j in range(2)]
    try:
        _options(lib, plans, fused, max_grid)
        lib.rns_fwd_mul_pair(plans, dc[0].ptr, dc[1].ptr, da.ptr, dk[0].ptr, dk[1].ptr, batch, flags, layout=lay)
        got_c, got_a, got_key = [d.download() for d in dc], da.download(), [d.download() for d in dk]
        if single:
            for j in range(2):
                da.upload(a_img), dc[j].upload(c_imgs[j])
                lib.rns_fwd_mul(plans, dc[j].ptr, da.ptr, dk[j].ptr, batch, flags, layout=lay)
                assert np.array_equal(dc[j].download(), got_c[j]), "c%d^ differs from the single call's" % j
    finally:
        da.free()
        for d in dc + dk:
            d.free()
        if own:
            for p in plans:
                p.destroy()
    want, fa = fwd_model(orc, primes, roots, a, keys, accs, n, batch, flags)
    cs = _check_pair(got_c, c_imgs, want, nl, n, batch, ls, ps, "fwd_mul_pair N=%d, batch %d, flags %d, %s" % (n, batch, flags, layout))
    after, used = rs.extract(got_a, nl, n, batch, ls, ps)
    assert np.array_equal(got_a[~used], a_img[~used]), "a word outside d_a changed"
    for j in range(2):
        assert np.array_equal(got_key[j], key_imgs[j]), "key%d changed" % j
    return cs, after, a, fa


def run_dot(lib, orc, primes, roots, n, batch, k, g, flags, layout="limb", seed=1, plans=None, extreme=False, single=False):
    """one ntt_rns_galois_dot_pair_batch call, every word of both outputs against galois_model.dot_model applied per component; the
    operands and the canaries untouched.  extreme: every operand word (and both c) is q - 1."""
    own = plans is None
    if own:
        plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    bc = bool(flags & gm.KEY_BROADCAST)
    nl = len(primes)

    def words(count, s):
        if extreme:
            return [np.full(count, q - 1, dtype=np.uint64) for q in primes]
        return [orc.fill_uniform(count, q, s * 1000 + l) for l, q in enumerate(primes)]

    a = [gm.operand(orc, primes, n, batch, seed + 10 * i) if not extreme else words(batch * n, 0) for i in range(k)]
    keys = [[words(n if bc else batch * n, seed + 10 * i + 5 + j * KEY1_SEED) for i in range(k)] for j in range(2)]
    c0 = [words(batch * n, seed + 7 + j * KEY1_SEED) for j in range(2)]
    pa = [gm.Placed(lib, x, n, batch, layout) for x in a]
    pk = [[gm.Placed(lib, x, n, batch, layout, bcast=bc) for x in keys[j]] for j in range(2)]
    pc = [gm.Placed(lib, c0[j], n, batch, layout) for j in range(2)]
    lay = gm._lay(layout, n, nl, batch)
    try:
        lib.rns_galois_dot_pair(plans, pc[0].ptr, pc[1].ptr, [x.ptr for x in pa], [x.ptr for x in pk[0]], [x.ptr for x in pk[1]], g, batch, flags,
                                layout=lay)
        got = []
        for j in range(2):
            limbs, clean = pc[j].download()
            assert clean, "a word outside output %d changed" % j
            got.append(limbs)
        assert all(x.unchanged() for x in pa + pk[0] + pk[1]), "an operand changed"
        if single:
            for j in range(2):
                one = gm.Placed(lib, c0[j], n, batch, layout)
                try:
                    lib.rns_galois_dot(plans, one.ptr, [x.ptr for x in pa], [x.ptr for x in pk[j]], g, batch, flags, layout=lay)
                    limbs, _ = one.download()
                finally:
                    one.free()
                for l in range(nl):
                    assert np.array_equal(limbs[l], got[j][l]), "output %d limb %d differs from the single call's" % (j, l)
    finally:
        for x in pa + pk[0] + pk[1] + pc:
            x.free()
        if own:
            for p in plans:
                p.destroy()
    for j in range(2):
        for l, q in enumerate(primes):
            want = gm.dot_model(orc, c0[j][l], [x[l] for x in a], [x[l] for x in keys[j]], n, g, q, flags)
            assert np.array_equal(got[j][l], want), "output %d limb %d of %d differs from the model (N=%d, batch %d, k %d, g %d, flags %d, %s)" % (
                j, l, nl, n, batch, k, g, flags, layout)
    return got


def untouched(ext, first, count):
    """the non-digit slots of d_ext that still hold the sentinel in every word"""
    return mm.untouched(ext, first, count)


def route(lib, orc):
    """2^14, 16 limbs of 50-bit primes (one run of the FP64 policy) and 2 of 60-bit primes, digit (0, 2), the fused pair kernel asked
    for: the FP64 run's slots of d_ext keep the sentinel"""
    n, first, count = 1 << 14, 0, 2
    primes, roots = rs.chain(lib, n, [50] * 16 + [60, 60])
    _, ext, _ = run(lib, orc, primes, roots, first, count, n, 2, BROADCAST | ACCUMULATE, fused=1, seed=17)
    assert untouched(ext, first, count)[:14] == list(range(2, 16)), "the FP64 run's slots of d_ext were written"
    print("key pair route: one call at 2^14 over 16 + 2 limbs")


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
    print("key pair launch proof: %d instances driven" % (driven + 1))


if __name__ == "__main__":
    main()
