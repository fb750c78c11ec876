"""GPU: fused_kernel<ArithF64, ...> computes at the 2^-1074 scale (ArithF64S, csrc/ntt_arith.h): every path of the kernel -- the
persistent forward and inverse loops, the two-halves 2^13 shape, the generic loop of the small blocks, lazy outputs, wide inputs,
the RNS (MULTI) instance, the block pass under a column pass and the pointer-table form -- bit for bit against the oracle through
the C ABI, on the input patterns that sit at the edges of the representation (zero, one non-zero word, q - 1 everywhere, the two
residues next to q / 2)."""
import numpy as np
import pytest

import kernel_recipes as kr

CLASSES = (0, 1, 18)
SIZES = (6, 9, 12, 13, 14)
BATCH = 5  # one polynomial per pattern; with NTT_OPT_MAX_GRID 2 the persistent loops wrap and 2^13's two halves see an odd count


def _patterns(oracle, n, q, seed):
    """[5][n]: random, all zero, a unit impulse, all q - 1, alternating (q - 1) / 2 and (q + 1) / 2"""
    a = np.zeros((BATCH, n), dtype=np.uint64)
    a[0] = oracle.fill_uniform(n, q, seed)
    a[2, n // 3] = 1
    a[3] = q - 1
    a[4, 0::2] = (q - 1) // 2
    a[4, 1::2] = (q + 1) // 2
    return a.reshape(-1)


def _lift(a, q):
    """the same residues anywhere in [0,8q)"""
    return a + np.uint64(q) * (np.arange(a.size, dtype=np.uint64) % np.uint64(8))


@pytest.mark.gpu
@pytest.mark.parametrize("ksh", CLASSES)
@pytest.mark.parametrize("m", SIZES)
def test_block_kernel_all_paths(lib, oracle, m, ksh):
    n = 1 << m
    (plan, q, cx), = kr.make_plans(lib, oracle, "ArithF64", ksh, n, 1)
    try:
        plan.set_option(lib.OPT_MAX_GRID, 2)
        a = _patterns(oracle, n, q, 0x5ca1ed + m)
        fwd, inv = cx.fwd(a), cx.inv(a)
        assert np.array_equal(plan.fwd_host(a), fwd), "forward"
        assert np.array_equal(plan.inv_host(a), inv), "inverse"
        lazy = plan.fwd_host(a, lazy=True)
        assert int(lazy.max()) < 4 * q and np.array_equal(lazy % np.uint64(q), fwd), "forward, lazy outputs"
        assert np.array_equal(plan.fwd_host(_lift(a, q), wide=True), fwd), "forward, wide inputs"
        assert np.array_equal(plan.inv_host(_lift(a, q), wide=True), inv), "inverse, wide inputs"
        assert np.array_equal(plan.inv_host(lazy, wide=True), a), "lazy words back through the inverse"
    finally:
        plan.destroy()


@pytest.mark.gpu
def test_rns_set_in_one_launch(lib, oracle):
    """3 limbs x 2 polynomials at 2^14: the MULTI instance"""
    n, batch = 1 << 14, 2
    ps = kr.make_plans(lib, oracle, "ArithF64", 0, n, 3)
    plans = [p for p, _, _ in ps]
    try:
        lib.set_rns_launch(plans, 0)
        # per limb: the random polynomial and one of the extreme ones
        a = np.concatenate([_patterns(oracle, n, q, 0xabc + i).reshape(BATCH, n)[[0, 3 + i % 2]].reshape(-1) for i, (_, q, _) in enumerate(ps)])
        for inverse in (False, True):
            buf = lib.DeviceBuffer(a.size).upload(a)
            try:
                (lib.rns_inv if inverse else lib.rns_fwd)(plans, buf.ptr, batch)
                got = buf.download()
            finally:
                buf.free()
            for i, (_, q, cx) in enumerate(ps):
                part = a[i * batch * n:(i + 1) * batch * n]
                assert np.array_equal(got[i * batch * n:(i + 1) * batch * n], cx.inv(part) if inverse else cx.fwd(part)), (i, inverse)
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
def test_block_pass_under_a_column_pass(lib, oracle):
    """2^16, 2 polynomials: the block pass reads the words the column pass (unit-scale policy) wrote, and the other way round"""
    n = 1 << 16
    (plan, q, cx), = kr.make_plans(lib, oracle, "ArithF64", 0, n, 1)
    try:
        # two launches: column_kernel over the leading two stages, fused_kernel over the 2^14-point blocks
        for o, v in (("OPT_BLOCK_LOG", 14), ("OPT_XCD_LOCAL", 0), ("OPT_ONE_PASS", 0), ("OPT_TWO_PHASE", 0)):
            plan.set_option(getattr(lib, o), v)
        a = oracle.fill_uniform(2 * n, q, 31)
        a[n:n + n // 2] = q - 1
        a[n + n // 2::2] = (q - 1) // 2
        a[n + n // 2 + 1::2] = (q + 1) // 2
        fwd = cx.fwd(a)
        assert np.array_equal(plan.fwd_host(a), fwd)
        assert np.array_equal(plan.inv_host(fwd), a)
    finally:
        plan.destroy()


@pytest.mark.gpu
def test_pointer_table_of_separate_allocations(lib, oracle):
    n = 1 << 14
    (plan, q, cx), = kr.make_plans(lib, oracle, "ArithF64", 0, n, 1)
    a = _patterns(oracle, n, q, 77).reshape(BATCH, n)[[0, 3, 4]]
    bufs = [lib.DeviceBuffer(n).upload(a[i]) for i in range(3)]
    try:
        plan.transform_ptrs([b.ptr for b in bufs])
        for i, b in enumerate(bufs):
            assert np.array_equal(b.download(), cx.fwd(a[i])), i
    finally:
        for b in bufs:
            b.free()
        plan.destroy()
