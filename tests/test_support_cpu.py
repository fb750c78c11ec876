"""CPU: the tests' own support layer -- tests/rns_support.py (prime chains, layouts with canaries) and tests/children.py (reading a
kernel trace's CSV; the rule that no child is started after one that did not end cleanly, on children that never load the library)."""
import os

import numpy as np
import pytest

import children
import rns_support as rs


def test_chain_over_the_oracle(oracle):
    n = 1 << 6
    primes, roots = rs.chain(oracle, n, [50, 50, 60])
    assert len(set(primes)) == 3
    assert [q.bit_length() for q in primes] == [50, 50, 60]
    for q, w in zip(primes, roots):
        assert q % (2 * n) == 1
        assert pow(w, n, q) == q - 1 and pow(w, 2 * n, q) == 1  # order exactly 2N (2N a power of two)


def test_chain_is_the_k_th_prime_of_each_bit_size(oracle):
    """what the per-file copies gave for a chain of tests/test_keyswitch_cpu.py: the k-th find_prime of a size at its k-th use"""
    n = 64
    primes, roots = rs.chain(oracle, n, [50] * 16 + [60])
    assert primes == [oracle.find_prime(50, n, k) for k in range(16)] + [oracle.find_prime(60, n, 0)]
    assert roots == [oracle.min_root(q, n) for q in primes]


def test_layouts_round_trip_among_canaries():
    n, nl, batch = 8, 3, 2
    limbs = [np.arange(batch * n, dtype=np.uint64) + np.uint64(100 * (l + 1)) for l in range(nl)]
    images = {}
    for kind in ("limb", "batch", "batch_padded", "limb_padded"):
        ls, ps, words = rs.layout_strides(kind, n, nl, batch)
        img = rs.place(limbs, n, batch, ls, ps, words)
        assert img.size == words
        got, used = rs.extract(img, nl, n, batch, ls, ps)
        assert int(used.sum()) == nl * batch * n  # no two polynomials overlap
        for l in range(nl):
            assert np.array_equal(got[l], limbs[l]), (kind, l)
        assert np.all(img[~used] == np.uint64(rs.CANARY)), kind
        images[kind] = img
    # every image is an array of its own: none shares memory with another or with the operand
    kinds = sorted(images)
    for i, a in enumerate(kinds):
        assert not any(np.shares_memory(images[a], c) for c in limbs)
        for b in kinds[i + 1:]:
            assert not np.shares_memory(images[a], images[b])


def test_trace_names_normalised_in_order_with_duplicates(tmp_path):
    mangled = "_ZN3ntt19rescale_coef_kernelEPmPKmmm"
    sub = tmp_path / "host" / "run"
    sub.mkdir(parents=True)
    with open(sub / "123_kernel_trace.csv", "w") as f:
        f.write('"Kind","Kernel_Name","Start_Timestamp"\n')
        for name in (mangled, "void ntt::rescale_fwd_kernel<ntt::ArithF64, 14, 1>(ntt::RescaleArgs)", mangled):
            f.write('"KERNEL_DISPATCH","%s",1\n' % name)
    names = children.trace_names(str(tmp_path))
    assert len(names) == 3 and names[0] == names[2] != names[1]
    assert names[0] == "rescale_coef_kernel" and names[1] == "rescale_fwd_kernel<ArithF64,14,1>", names


def test_trace_names_without_a_csv(tmp_path):
    with pytest.raises(AssertionError, match="wrote no CSV"):
        children.trace_names(str(tmp_path))


def test_no_child_is_started_after_one_that_did_not_end_cleanly(tmp_path):
    """host-only children (they never load the library): a child at its time limit trips the rule, the next one is not started, a
    failed assertion alone does not trip it"""
    mark = os.path.join(str(tmp_path), "started")
    before = list(children._UNCLEAN)  # (a real child that did not end cleanly earlier in the session keeps barring the rest)
    children._reset()
    try:
        with pytest.raises(pytest.fail.Exception):
            children.python_child("import time; time.sleep(5)", seconds=1)
        with pytest.raises(pytest.fail.Exception, match="not started"):
            children.python_child("open(%r, 'w').close(); print('x')" % mark, marker="x")
        assert not os.path.exists(mark)
        children._reset()
        with pytest.raises(AssertionError, match="exit 1"):
            children.python_child("raise AssertionError('no')")
        children.python_child("open(%r, 'w').close(); print('x')" % mark, marker="x")
        assert os.path.exists(mark)
    finally:
        children._reset()
        children._UNCLEAN.extend(before)
