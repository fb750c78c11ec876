"""GPU: the ciphertext tensor product and ModDown into a ciphertext (ntt_rns_tensor_batch, ntt_rns_mod_down_add_batch and their strided
forms).  Every output word against the model of tests/ct_mul_model.py, exactly: the tensor over sizes, batches, the 16-limb launch
boundary, a mixed chain, the extremes of the canonical and of the lazy range, squaring and in-place by aliasing, layouts with
canaries; every ksfold_fwd_kernel instance with 1 and 3 P primes, with and without accumulation, the accumulator's contract
included; the composition route (integer-policy limbs, coefficients, N >= 2^15, option 0) and fused == composition; argument errors
that write nothing; the plain-C example of a whole multiplication; and two kernel traces: the fused route at 2^14 over 16 + 2 limbs
and the launch of all 38 new instances."""
import os
import re

import numpy as np
import pytest

import children
import ct_mul_model as cm
import kernel_inventory
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "ct_mul_model.py")
T, F, A = cm.TRANSFORMED, cm.FLOOR, cm.ACCUMULATE
MIXED = [60, 50, 30, 52]


# ---------------------------------------------------------------- tensor

@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [1, 17])
@pytest.mark.parametrize("batch", [1, 3, 130])
@pytest.mark.parametrize("logn", [1, 6, 12])
def test_tensor_shapes(lib, oracle, logn, batch, nlimbs):
    n = 1 << logn
    primes, _ = rs.chain(lib, n, [50] * nlimbs)
    cm.run_tensor(lib, oracle, primes, n, batch, cm.tensor_inputs(oracle, primes, n, batch, logn + batch))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "zero", "max", "lazy60", "lazy30"])
def test_tensor_mixed_chain_and_extremes(lib, oracle, case):
    """60-, 50-, 30- and 52-bit limbs take the same integer kernel; all-zero and all-(q-1) words; with NTT_MUL_LAZY_IN all-(4q-1) words
    on the 60-bit and on the 30-bit limb"""
    n, batch = 1 << 12, 3
    primes, _ = rs.chain(lib, n, MIXED)
    lazy = {"lazy60": (0,), "lazy30": (2,)}.get(case, ())
    ops = cm.tensor_inputs(oracle, primes, n, batch, 9, fill=case if case in ("zero", "max") else None, lazy_limbs=lazy)
    cm.run_tensor(lib, oracle, primes, n, batch, ops, flags=cm.LAZY_IN if lazy else 0)


@pytest.mark.gpu
def test_tensor_squaring_and_in_place_by_aliasing(lib, oracle):
    n, batch = 1 << 10, 3
    primes, _ = rs.chain(lib, n, MIXED)
    ops = cm.tensor_inputs(oracle, primes, n, batch, 21)
    square = cm.run_tensor(lib, oracle, primes, n, batch, ops, mode="square")
    general = cm.run_tensor(lib, oracle, primes, n, batch, [ops[0], ops[1], [v.copy() for v in ops[0]], [v.copy() for v in ops[1]]])
    for x, y in zip(square, general):
        for u, v in zip(x, y):
            assert np.array_equal(u, v), "the squaring path differs from the general path"
    cm.run_tensor(lib, oracle, primes, n, batch, ops, mode="inplace")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded", "odd_limb_stride"])
def test_tensor_layouts(lib, oracle, layout):
    n, batch = 1 << 11, 3
    primes, _ = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    if layout == "odd_limb_stride":
        ls = batch * n + 1
        layout = (ls, n, (len(primes) - 1) * ls + batch * n + 8)
    cm.run_tensor(lib, oracle, primes, n, batch, cm.tensor_inputs(oracle, primes, n, batch, 13), layout=layout)


# ---------------------------------------------------------------- ModDown-add, the fused kernel

@pytest.mark.gpu
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
@pytest.mark.parametrize("np_", [1, 3])
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn, np_, acc):
    """each ksfold_fwd_kernel<policy, LOGN, class>: three Q limbs of the class, np 60-bit P limbs, batch 3 (the tail of a workgroup
    that serves several blocks), round (even LOGN) / floor (odd); the accumulator's Q limbs unchanged, its P limbs in coefficients"""
    n = 1 << logn
    b = rs.CLASS_BITS[(pol, k)]
    primes, roots = rs.chain(lib, n, [b] * 3 + [60] * np_)
    flags = T | acc | (F if logn % 2 else 0)
    cm.run_down_add(lib, oracle, primes, roots, np_, n, 3, flags, fused=1, seed=logn + np_, a_untouched=True)


# ---------------------------------------------------------------- ModDown-add, the other routes

@pytest.mark.gpu
@pytest.mark.parametrize("nq", [5, 17, 18, 34])
@pytest.mark.parametrize("flags", [A, T | A, T])
@pytest.mark.parametrize("fused", [None, 0])
def test_q_counts_across_the_run_boundary(lib, oracle, nq, flags, fused):
    n = 1 << 8
    primes, roots = rs.chain(lib, n, [50] * nq + [60, 60, 60])
    cm.run_down_add(lib, oracle, primes, roots, 3, n, 2, flags, fused=fused, seed=nq)


@pytest.mark.gpu
@pytest.mark.parametrize("qbits,pbits", [([60, 50, 50, 52, 50, 30], [60, 60]), ([52, 52, 50], [60]), ([50, 50, 51], [52, 52, 52]),
                                         ([60, 30], [50, 50]), ([30, 30, 30, 30], [52] * 16)],
                         ids=["60-50-52-30", "52-bit", "p52", "60-30", "p16"])
@pytest.mark.parametrize("flags", [0, F, T, T | F])
@pytest.mark.parametrize("acc", [0, A], ids=["store", "accumulate"])
def test_mixed_chains(lib, oracle, qbits, pbits, flags, acc):
    """integer-policy runs between FP64 runs; the coefficient domain (flags 0 and F)"""
    n = 1 << 12
    primes, roots = rs.chain(lib, n, qbits + pbits)
    cm.run_down_add(lib, oracle, primes, roots, len(pbits), n, 3, flags | acc, seed=len(qbits))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["auto", "u64", "r4"])
@pytest.mark.parametrize("flags", [A, T | A, T | F])
def test_integer_policy_limbs(lib, oracle, arith, flags):
    n = 1 << 12
    a = {"auto": lib.ARITH_AUTO, "u64": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[arith]
    primes, roots = rs.chain(lib, n, [58] * 5 if arith != "auto" else [60] * 5)
    plans = [lib.Plan(n, q, w, arith=a) for q, w in zip(primes, roots)]
    try:
        cm.run_down_add(lib, oracle, primes, roots, 2, n, 3, flags, plans=plans, seed=7)
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 16])
def test_composition_at_large_sizes(lib, oracle, logn):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50, 50, 60])
    cm.run_down_add(lib, oracle, primes, roots, 1, n, 2, T | A, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,nq,np_", [(14, 16, 2), (9, 5, 1), (12, 20, 3)])
def test_fused_equals_composition_bit_for_bit(lib, oracle, logn, nq, np_):
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [50] * nq + [60] * np_)
    fused = cm.run_down_add(lib, oracle, primes, roots, np_, n, 2, T | A, fused=1, seed=3, a_untouched=True)
    comp = cm.run_down_add(lib, oracle, primes, roots, np_, n, 2, T | A, fused=0, seed=3)
    sandwich = cm.run_down_add(lib, oracle, primes, roots, np_, n, 2, T | A, fused=0, rescale_fused=0, seed=3, cross_check=False)
    for x, y, z in zip(fused, comp, sandwich):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.gpu
@pytest.mark.parametrize("c_layout,a_layout", [("batch", "batch"), ("batch_padded", "batch_padded"), ("limb", "limb"), ("limb_padded", "batch")])
@pytest.mark.parametrize("flags", [A, T | A, T | F])
@pytest.mark.parametrize("fused", [None, 0])
def test_layouts(lib, oracle, c_layout, a_layout, flags, fused):
    n = 1 << 11
    primes, roots = rs.chain(lib, n, [50, 50, 50, 52, 60, 60])
    cm.run_down_add(lib, oracle, primes, roots, 2, n, 3, flags, c_layout=c_layout, a_layout=a_layout, fused=fused, seed=11)


# ---------------------------------------------------------------- argument errors

@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 10, 2
    primes, roots = rs.chain(lib, n, [50] * 18)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    q2 = lib.find_prime(50, 2 * n)
    other = lib.Plan(2 * n, q2, lib.min_root(q2, 2 * n))
    same = lib.Plan(n, primes[0], roots[0])
    fwd_only = rs.forward_only_plan(lib, n, primes[3], roots[3])
    fwd_only_q = rs.forward_only_plan(lib, n, primes[1], roots[1])
    words = 18 * batch * n
    pat = oracle.fill_uniform(2 * words, primes[0], 5)
    buf = lib.DeviceBuffer(2 * words).upload(pat)
    a_ptr, c_ptr = buf.ptr, buf.ptr + 8 * words
    p4 = plans[:4]
    per = 4 * batch * n  # words of a four-limb operand

    def refused(what, call):
        with pytest.raises(lib.NttError):
            call()
        assert np.array_equal(buf.download(), pat), what

    def down(ps, np_, flags, lay=None, c=c_ptr, a=a_ptr):
        return lambda: lib.rns_mod_down_add(ps, np_, c, a, batch, flags, layout=lay)

    refused("no Q limb", down(plans[:2], 2, T))
    refused("no P limb", down(plans[:2], 0, T))
    refused("17 P limbs", down(plans[:18], 17, 0))
    refused("differing N", down([plans[0], other, plans[2], plans[3]], 2, T))
    refused("a prime twice", down([plans[0], plans[1], plans[2], same], 2, 0))
    refused("unknown flag", down(p4, 2, 8))
    refused("overlapping strides of a", down(p4, 2, T, (batch * n, n, n, n)))
    refused("overlapping strides of c", down(p4, 2, T, (n, n, batch * n, n)))
    refused("null c", down(p4, 2, T, c=None))
    refused("null a", down(p4, 2, T, a=None))
    refused("c inside a", down(p4, 2, T, c=a_ptr + 8 * n))
    refused("c overlapping a's tail", down(p4, 2, T, c=a_ptr + 8 * (per - n)))
    refused("P limb without its inverse table", down([plans[0], plans[1], plans[2], fwd_only], 2, T))
    # a Q limb without the inverse table: refused where the sandwich would serve it, served by the fused kernels
    ps = [plans[0], fwd_only_q, plans[2], plans[3]]
    plans[0].set_option(lib.OPT_MODDOWN_ADD_FUSED, 0)
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 0)
    refused("sandwich without an inverse table", down(ps, 2, T | A))
    plans[0].set_option(lib.OPT_RESCALE_FUSED, 1)
    plans[0].set_option(lib.OPT_MODDOWN_ADD_FUSED, -1)
    cm.run_down_add(lib, oracle, primes[:4], roots[:4], 2, n, batch, T | A, plans=ps, fused=1, seed=9, cross_check=False)
    # the in-place call keeps refusing the new flag
    refused("ACCUMULATE passed to ntt_rns_mod_down_batch", lambda: lib.rns_mod_down(p4, 2, a_ptr, batch, T | A))

    t3 = plans[:3]
    span = 3 * batch * n
    o = [buf.ptr + 8 * i * span for i in range(7)]  # seven disjoint three-limb operands inside the buffer

    def tensor(ps, ptrs, flags=0, lay=None):
        return lambda: lib.rns_tensor(ps, *ptrs, batch, flags, layout=lay)

    refused("no limb", tensor([], o))
    refused("differing N", tensor([plans[0], other, plans[2]], o))
    refused("unknown flag", tensor(t3, o, 2))
    refused("accumulate flag", tensor(t3, o, 4))
    refused("overlapping strides", tensor(t3, o, 0, (n, n)))
    for i in range(7):
        refused("null pointer %d" % i, tensor(t3, o[:i] + [None] + o[i + 1:]))
    refused("c0 overlaps c1", tensor(t3, [o[0], o[0] + 8 * n] + o[2:]))
    refused("c0 is c2", tensor(t3, [o[0], o[1], o[0]] + o[3:]))
    refused("c1 overlaps a0, shifted", tensor(t3, [o[0], o[3] + 8, o[2]] + o[3:]))
    refused("c2 overlaps b1, shifted", tensor(t3, o[:2] + [o[6] - 8 * n] + o[3:6] + [o[6]]))
    for p in plans + [other, same, fwd_only, fwd_only_q]:
        p.destroy()
    buf.free()


# ---------------------------------------------------------------- the example

@pytest.mark.gpu
def test_example_checksums_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_ciphertext_mul")
    got = {(int(m.group(1)), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r"comp (\d+) limb (\d+) q \d+ checksum ([0-9a-f]+)", out)}
    want = cm.example_model(lib, oracle)
    assert len(got) == 14 and got == want, sorted(k for k in want if got.get(k) != want[k])


# ---------------------------------------------------------------- launch proofs

@pytest.mark.gpu
def test_route_proof_p_inverses_and_one_fused_launch():
    """2^14, 16 Q limbs of 50-bit primes and 2 P limbs of 60-bit primes, NTT domain, accumulating: the call launches the inverse
    transforms of the P limbs and exactly one ksfold_fwd_kernel, nothing else"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in rs.SETUP_KERNELS]
    fused = [k for k in launched if k.startswith("ksfold_fwd_kernel")]
    assert fused == ["ksfold_fwd_kernel<ArithF64,14,1>"], launched
    others = [k for k in launched if not k.startswith("ksfold_fwd_kernel")]
    assert others and all(kernel_inventory.parse(k).args.get("INV") is True for k in others), launched
    assert launched[-1] == fused[0], launched


@pytest.mark.gpu
def test_launch_proof_every_new_instance():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = rs.kernel_names("ksfold_fwd_kernel", rs.fused_launch_cases()) | {"tensor_kernel", "ct_fold_kernel"}
    assert len(want) == 38
    assert not sorted(want - launched), "instances never launched: %s" % sorted(want - launched)
