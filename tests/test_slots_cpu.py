"""CPU: the statements of the BFV / BGV slot order (include/ntt_mi355x.h, csrc/ntt_slots.h) checked on the model of
tests/slots_model.py against the oracle: pos is a permutation; decode is the evaluation at psi^e(i); decode(encode(v)) = v; products of
polynomials are slot-wise products; sigma_g with g = 5^r rotates both rows left by r and g = 2N - 1 swaps them, through both forms of
the Galois model (coefficients and NTT domain); the host's ntt_slot_position; and the plain-C example compiles against the public
header.  N = 2, 4, 8, 64, 1024 and 2^15 with a fitting prime t each (t = 5, 17, 97, 257, 65537 among them)."""
import os
import subprocess

import numpy as np
import pytest

import galois_model as gm
import slots_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 5), (4, 17), (8, 97), (64, 257), (1024, 65537), (1 << 15, 65537)]
IDS = ["N%d-t%d" % c for c in CASES]


@pytest.fixture(scope="module")
def ctxs(oracle):
    """one oracle context and one vector of slot words per case, shared by the tests and left unchanged"""
    out = {}
    for n, t in CASES:
        assert oracle.lib.orc_is_prime(t) and (t - 1) % (2 * n) == 0
        cx = oracle.ctx(n, t, oracle.min_root(t, n))
        out[(n, t)] = (cx, sm.words(oracle, n, t, 2, n), sm.words(oracle, n, t, 2, n + 1))
    return out


@pytest.mark.parametrize("n,t", CASES, ids=IDS)
def test_pos_is_a_permutation(n, t):
    pos = sm.pos_table(n)
    assert np.array_equal(np.sort(pos), np.arange(n))
    assert np.array_equal(pos[sm.ipos_table(n)], np.arange(n))
    if n == 2:
        assert pos.tolist() == [0, 1]


@pytest.mark.parametrize("n,t", [c for c in CASES if c[0] <= 64], ids=[i for c, i in zip(CASES, IDS) if c[0] <= 64])
def test_decode_is_the_evaluation_at_the_slot_roots(ctxs, n, t):
    cx, v, _ = ctxs[(n, t)]
    a = v[:n]
    got = sm.decode(cx, a)
    psi = cx.root
    for i, e in enumerate(sm.exponents(n)):
        x = pow(psi, e, t)
        assert int(got[i]) == sum(int(c) * pow(x, k, t) for k, c in enumerate(a)) % t, i


@pytest.mark.parametrize("n,t", CASES, ids=IDS)
def test_round_trip(ctxs, n, t):
    cx, v, _ = ctxs[(n, t)]
    a = sm.encode(cx, v)
    assert int(a.max()) < t
    assert np.array_equal(sm.decode(cx, a), v)
    assert np.array_equal(sm.encode(cx, sm.decode(cx, v)), v)


@pytest.mark.parametrize("n,t", CASES, ids=IDS)
def test_products_are_slot_wise(oracle, ctxs, n, t):
    """through Oracle.schoolbook up to N = 1024; at 2^15 (2^30 products per polynomial) through the oracle's own transforms"""
    cx, v1, v2 = ctxs[(n, t)]
    a, b = sm.encode(cx, v1[:n]), sm.encode(cx, v2[:n])
    if n <= 1024:
        c = oracle.schoolbook(a, b, n, t)
    else:
        c = cx.inv(oracle.pointwise(cx.fwd(a), cx.fwd(b), t))
    assert np.array_equal(sm.decode(cx, c), oracle.pointwise(v1[:n], v2[:n], t))


@pytest.mark.parametrize("n,t", CASES, ids=IDS)
@pytest.mark.parametrize("r", [1, 3, -1])
def test_rotation_by_the_powers_of_five(ctxs, n, t, r):
    cx, v, _ = ctxs[(n, t)]
    g = gm.rotation(n, r)
    want = sm.rotate_rows(v, n, r)
    a = sm.encode(cx, v)
    assert np.array_equal(sm.decode(cx, gm.coef_model(a, n, g, t)), want)
    hat = gm.ntt_model(cx.fwd(a), n, g).reshape(-1, n)
    assert np.array_equal(hat[:, sm.pos_table(n)].reshape(-1), want)
    if n >= 16:
        assert not np.array_equal(want, v)


@pytest.mark.parametrize("n,t", CASES, ids=IDS)
def test_conjugation_swaps_the_rows(ctxs, n, t):
    cx, v, _ = ctxs[(n, t)]
    g = 2 * n - 1
    want = sm.swap_rows(v, n)
    a = sm.encode(cx, v)
    assert np.array_equal(sm.decode(cx, gm.coef_model(a, n, g, t)), want)
    hat = gm.ntt_model(cx.fwd(a), n, g).reshape(-1, n)
    assert np.array_equal(hat[:, sm.pos_table(n)].reshape(-1), want)


def test_host_slot_position_matches_the_model(lib):
    for n in (2, 4, 64, 1 << 15):
        pos = sm.pos_table(n)
        idx = range(n) if n <= 64 else list(range(0, n, 997)) + [n // 2 - 1, n // 2, n - 1]
        for i in idx:
            assert lib.slot_position(n, i) == int(pos[i]), (n, i)
    for n, i in ((0, 0), (1, 0), (3, 1), (96, 5), (8, 8), (8, 1 << 40)):
        assert lib.slot_position(n, i) is None, (n, i)


def test_example_compiles_against_the_public_header():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rns_slots.c")])
