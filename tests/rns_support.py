"""Support shared by the RNS models (tests/*_model.py) and their tests: prime chains, the FP64 class table and the instance list of
the prologue-fused kernels, operand layouts with canaries, the edge words, plan lists, and the loader of script mode.  Pure helpers:
nothing here starts a process (that is tests/children.py) and nothing needs a GPU to import."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a model run as a script (`python3 tests/x_model.py`) has tests/ on its path already; the binding lives one level up
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def load():
    """(the library binding, the oracle): the preamble of every model's main()"""
    import ontt
    from oracle_binding import Oracle
    return ontt.load(), Oracle()


def chain(finder, n, bits_list):
    """distinct primes = 1 mod 2n of the given bit sizes (in order) and their minimal roots; finder: the library binding or the
    oracle (both have find_prime and min_root)"""
    seen, primes = {}, []
    for b in bits_list:
        k = seen.get(b, 0)
        primes.append(finder.find_prime(b, n, k))
        seen[b] = k + 1
    return primes, [finder.min_root(q, n) for q in primes]


# the bit sizes that land a 2^6..2^14 plan in each FP64 policy / headroom class (ntt_tables.h h_f64_ksh, host_plan.inc kcls)
CLASS_BITS = {("ArithF64", 0): 51, ("ArithF64", 1): 50, ("ArithF64", 18): 30, ("ArithF64W", 0): 52}
LOGNS = range(6, 15)


def fused_launch_cases():
    """(policy, class, logn) of every instance of a prologue-fused forward kernel (rescale_fwd_kernel, moddown_fwd_kernel, ...)"""
    return [(pol, k, logn) for (pol, k) in CLASS_BITS for logn in LOGNS]


def kernel_names(prefix, cases):
    """the normalised names prefix<policy,LOGN,class> of (policy, class, logn) cases"""
    return {"%s<%s,%d,%d>" % (prefix, pol, logn, k) for pol, k, logn in cases}


# kernels a plan's creation launches (table builds): not part of a call
SETUP_KERNELS = ("power_table_kernel", "records_u64_kernel", "records_f64_kernel", "records_r4_kernel")


def u64(a):
    return np.asarray(a, dtype=np.uint64)


def full(n, v):
    return np.full(n, v, dtype=np.uint64)


def edge_fill(a, q):
    """the extremes of the canonical range in the first four words"""
    a[:4] = [0, q - 1, (q - 1) // 2, (q + 1) // 2]


def layout_strides(kind, n, nlimbs, batch):
    """(limb_stride, poly_stride, words) of a layout: [limb][batch][N], [batch][limb][N] or padded forms of either"""
    if kind == "limb":
        return batch * n, n, nlimbs * batch * n
    if kind == "batch":
        return n, nlimbs * n, nlimbs * batch * n
    if kind == "batch_padded":
        ls, ps = n + 64, nlimbs * (n + 64) + 128
        return ls, ps, (batch - 1) * ps + (nlimbs - 1) * ls + n + 96
    if kind == "limb_padded":
        ls, ps = batch * (n + 32) + 256, n + 32
        return ls, ps, (nlimbs - 1) * ls + (batch - 1) * ps + n + 96
    raise ValueError(kind)


CANARY = 0xC0FFEE5EEDC0FFEE


def place(limbs, n, batch, ls, ps, words):
    """host image of an operand: limb l, polynomial p at l * ls + p * ps; every other word a canary"""
    img = np.full(words, CANARY, dtype=np.uint64)
    for l, c in enumerate(limbs):
        for p in range(batch):
            img[l * ls + p * ps:l * ls + p * ps + n] = c[p * n:(p + 1) * n]
    return img


def extract(img, nlimbs, n, batch, ls, ps):
    """(limbs, mask of the words the operand occupies)"""
    used = np.zeros(img.size, dtype=bool)
    out = []
    for l in range(nlimbs):
        parts = []
        for p in range(batch):
            o = l * ls + p * ps
            parts.append(img[o:o + n])
            used[o:o + n] = True
        out.append(np.concatenate(parts))
    return out, used


def plans(lib, n, primes, roots, arith=None):
    return [lib.Plan(n, q, w) if arith is None else lib.Plan(n, q, w, arith=arith) for q, w in zip(primes, roots)]


def forward_only_plan(lib, n, q, w):
    """a plan built from the forward table alone (no inverse): ntt_plan_create_from_tables with w_inv_powers = NULL"""
    logn = n.bit_length() - 1
    rev = [int(format(i, "0%db" % logn)[::-1], 2) if logn else 0 for i in range(n)]
    powers = np.array([pow(w, r, q) for r in rev], dtype=np.uint64)
    h = C.c_void_p()
    rc = lib._lib.ntt_plan_create_from_tables(C.byref(h), 0, n, q, powers.ctypes.data_as(lib.U64P), None, lib.ARITH_AUTO)
    assert rc == 0, lib._lib.ntt_last_error()
    p = object.__new__(lib.Plan)
    p.h, p.N, p.q, p.root, p.device = h.value, n, q, w, 0
    return p
