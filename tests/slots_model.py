"""Model of the BFV / BGV slot encode and decode (ntt_slots_encode_batch, ntt_slots_decode_batch) for the tests, in numpy and Python
integers; nothing of the kernels' index code: pos comes from pow(5, j, 2N) and a bit reversal by a loop, encode and decode go through
the oracle's Ctx.inv / Ctx.fwd.

    slot i = r h + j (row r, column j < h = N / 2);  e(i) = 5^j mod 2N (r = 0), 2N - 5^j mod 2N (r = 1);  pos(i) = bitrev_m((e(i) - 1) / 2)
    decode  v[i] = fwd(a)[pos(i)];   encode  a = inv(a^), a^[pos(i)] = v[i]

The case runners of tests/test_gpu_slots.py place both sides among canaries (galois_model.Placed) and check the output word for word,
the canaries and, for encode, the input for being untouched.

Script mode (a fresh process under a kernel trace): `python3 tests/slots_model.py --route` runs one fused encode and one fused decode at
2^14 x 4; without arguments every new kernel instance is launched once, each checked.
"""
import sys

import numpy as np

import galois_model as gm
import rns_support as rs

OPT_MAX_GRID, OPT_F64_CLASS, OPT_SLOTS_FUSED = 1, 3, 23
SETUP_KERNELS = rs.SETUP_KERNELS + ("slots_table_kernel",)


def bitrev_int(x, m):
    y = 0
    for _ in range(m):
        y = (y << 1) | (x & 1)
        x >>= 1
    return y


def exponents(n):
    """e(i) for every slot i < n"""
    h = n // 2
    row0 = [pow(5, j, 2 * n) for j in range(h)]
    return row0 + [2 * n - e for e in row0]


def pos_table(n):
    """pos(i) for every slot i < n = 2^m"""
    m = n.bit_length() - 1
    return np.array([bitrev_int((e - 1) // 2, m) for e in exponents(n)], dtype=np.int64)


def ipos_table(n):
    ip = np.zeros(n, dtype=np.int64)
    ip[pos_table(n)] = np.arange(n, dtype=np.int64)
    return ip


def _polys(a, n):
    return np.asarray(a, dtype=np.uint64).reshape(-1, n)


def decode(cx, a):
    """the slots of [batch][N] coefficient polynomials (cx: the oracle's context for (N, t, psi))"""
    return _polys(cx.fwd(a), cx.N)[:, pos_table(cx.N)].reshape(-1)


def encode(cx, v):
    """the [batch][N] polynomials whose slots are v"""
    hat = np.zeros_like(_polys(v, cx.N))
    hat[:, pos_table(cx.N)] = _polys(v, cx.N)
    return cx.inv(hat.reshape(-1))


def rotate_rows(v, n, r):
    """both rows rotated left by r: new (row, j) holds the old (row, (j + r) mod h)"""
    h = n // 2
    j = (np.arange(h) + r) % h
    src = np.concatenate([j, h + j])
    return _polys(v, n)[:, src].reshape(-1)


def swap_rows(v, n):
    h = n // 2
    return _polys(v, n)[:, np.concatenate([np.arange(h, n), np.arange(h)])].reshape(-1)


def corner_words(t):
    return [0, 1 % t, t - 1, (t - 1) // 2, (t + 1) // 2]


def words(orc, n, t, batch, seed, extreme=False):
    """[batch][N] canonical words mod t with the corner words in the first slots of every polynomial; extreme: every word t - 1"""
    if extreme:
        return np.full(batch * n, t - 1, dtype=np.uint64)
    v = orc.fill_uniform(batch * n, t, 7000 + seed).reshape(batch, n)
    c = corner_words(t)[:n]
    v[:, :len(c)] = c
    return v.reshape(-1)


def plan_for(lib, n, t, root=None, arith=None, fused=None, max_grid=0, f64_class=None):
    p = lib.Plan(n, t, root if root else lib.min_root(t, n), arith=lib.ARITH_AUTO if arith is None else arith)
    p.enable_slots()
    if fused is not None:
        p.set_option(OPT_SLOTS_FUSED, fused)
    if max_grid:
        p.set_option(OPT_MAX_GRID, max_grid)
    if f64_class is not None:
        p.set_option(OPT_F64_CLASS, f64_class)
    return p


def _strides(n, batch, pad):
    """(stride, words) of a one-limb operand: dense, or padded with room behind the last polynomial"""
    return (n, batch * n) if not pad else (n + pad, (batch - 1) * (n + pad) + n + 40)


class Side:
    """[batch][N] words uploaded `stride` words apart among canaries"""

    def __init__(self, lib, data, n, batch, pad):
        self.n, self.batch = n, batch
        self.ps, self.words = _strides(n, batch, pad)
        self.img = rs.place([np.asarray(data, dtype=np.uint64)], n, batch, 0, self.ps, self.words)
        self.buf = lib.DeviceBuffer(self.words).upload(self.img)
        self.ptr = self.buf.ptr

    def download(self):
        got = self.buf.download()
        limbs, used = rs.extract(got, 1, self.n, self.batch, 0, self.ps)
        return limbs[0], np.array_equal(got[~used], self.img[~used])

    def unchanged(self):
        return np.array_equal(self.buf.download(), self.img)

    def free(self):
        self.buf.free()


def run_case(lib, orc, n, t, batch, direction, fused=None, v_pad=0, a_pad=0, max_grid=0, arith=None, f64_class=None, seed=1, extreme=False,
             plan=None):
    """one call (direction "encode" or "decode") on words with the corners in front, every output word against the model; the canaries
    on both sides and -- encode -- the input untouched.  Returns the output words."""
    own = plan is None
    root = lib.min_root(t, n) if own else plan.root
    if own:
        plan = plan_for(lib, n, t, root, arith, fused, max_grid, f64_class)
    cx = orc.ctx(n, t, root)
    src = words(orc, n, t, batch, seed, extreme)
    want = encode(cx, src) if direction == "encode" else decode(cx, src)
    pads = (v_pad, a_pad) if direction == "encode" else (a_pad, v_pad)
    s_in = Side(lib, src, n, batch, pads[0])
    s_out = Side(lib, np.full(batch * n, 0xDEAD, dtype=np.uint64), n, batch, pads[1])
    lay = None if not (v_pad or a_pad) else ((s_in.ps, s_out.ps) if direction == "encode" else (s_out.ps, s_in.ps))
    try:
        if direction == "encode":
            lib.slots_encode(plan, s_out.ptr, s_in.ptr, batch, layout=lay)
            assert s_in.unchanged(), "encode changed its input"
        else:
            lib.slots_decode(plan, s_out.ptr, s_in.ptr, batch, layout=lay)
            _, clean_in = s_in.download()
            assert clean_in, "a word outside the consumed operand changed"
        got, clean = s_out.download()
        assert clean, "a word outside the output changed"
    finally:
        s_in.free(), s_out.free()
        if own:
            plan.destroy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s differs from the model at %d of %d words, first %d (N=%d, t=%d, batch %d, fused %s, pads %d/%d, grid %d)" % (
        direction, bad.size, got.size, bad[0], n, t, batch, fused, v_pad, a_pad, max_grid)
    return got


# ---------------------------------------------------------------- kernel instances

def class_modulus(lib, pol, k, n):
    """a prime t = 1 mod 2n whose plan lands in the class: 30, 50, 51 and 52 bits (rns_support.CLASS_BITS)"""
    return lib.find_prime(rs.CLASS_BITS[(pol, k)], n)


def run_instance(lib, orc, pol, k, logn):
    """both kernels of one instance: batch 3 (below 2^9 a partly dead group of sub-blocks; at 2^13 an idle half)"""
    n = 1 << logn
    t = class_modulus(lib, pol, k, n)
    plan = plan_for(lib, n, t, fused=1)
    info = plan.info()
    assert info["f64_class"] == (52 if pol == "ArithF64W" else k), (pol, k, info)
    try:
        run_case(lib, orc, n, t, 3, "encode", plan=plan, seed=logn)
        run_case(lib, orc, n, t, 3, "decode", plan=plan, seed=logn + 1)
    finally:
        plan.destroy()


def kernel_names():
    out = {"slots_perm_kernel", "slots_table_kernel"}
    for pol, k, logn in rs.fused_launch_cases():
        out |= {"slots_inv_kernel<%s,%d,%d>" % (pol, logn, k), "slots_fwd_kernel<%s,%d,%d>" % (pol, logn, k)}
    return out


def route(lib, orc):
    """2^14 x 4, t = 65537, the fused route: one encode, one decode"""
    n, t = 1 << 14, 65537
    plan = plan_for(lib, n, t, fused=1)
    run_case(lib, orc, n, t, 4, "encode", plan=plan, seed=14)
    run_case(lib, orc, n, t, 4, "decode", plan=plan, seed=15)
    plan.destroy()
    print("slots route: one fused encode and one fused decode at 2^14 x 4")


# ---------------------------------------------------------------- the example

def example_model(lib, orc):
    """the lines examples/rns_slots.c prints"""
    n, t, steps = 1 << 12, 65537, 3
    v1, v2 = orc.fill_uniform(n, t, 1), orc.fill_uniform(n, t, 2)
    want = rotate_rows(orc.pointwise(v1, v2, t), n, steps)
    s = "%016x" % orc.checksum(want)
    return ["decoded checksum " + s, "expected checksum " + s, "decoded == slot-wise product rotated left by 3: yes"]


def main():
    lib, orc = rs.load()
    if "--route" in sys.argv[1:]:
        route(lib, orc)
        return
    for pol, k, logn in rs.fused_launch_cases():
        run_instance(lib, orc, pol, k, logn)
    run_case(lib, orc, 1 << 5, 65537, 2, "encode", seed=5)
    print("slots launch proof: %d instances driven" % (2 * len(rs.fused_launch_cases()) + 2))


if __name__ == "__main__":
    main()
