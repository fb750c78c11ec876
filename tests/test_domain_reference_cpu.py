"""CPU: the references of the NTT-domain product recipes (tests/kernel_recipes.py: dot_reference, mul_reference) against schoolbook
negacyclic products in Python integers.

The recipes form want = inv(sum_i a_i^ (.) b_i^) and want = fwd(a) (.) b^ (+ c^) with the oracle's transforms.  Here every
transformed operand is taken back to coefficients by the defining sum of the inverse transform -- a[j] = N^-1 sum_i a^[bitrev(i)]
psi^-((2i+1) j), Python integers, no butterflies and none of the oracle's code -- and the products are sums over i + j with the sign
of X^N = -1.  N = 2^6 and 2^8, an FP64-class prime and a 60-bit prime, k = 3."""
import numpy as np
import pytest

import kernel_recipes

BATCH, K = 2, 3


def _bitrev(i, m):
    return int(format(i, "0%db" % m)[::-1], 2)


def _inverse_by_definition(ahat, n, q, psi):
    """coefficients of one polynomial given in the NTT domain (bit-reversed order: a^[bitrev(i)] = a(psi^(2i+1)))"""
    m = n.bit_length() - 1
    ninv, ipsi = pow(n, -1, q), pow(psi, -1, q)
    vals = [int(ahat[_bitrev(i, m)]) % q for i in range(n)]
    out = []
    for j in range(n):
        step, p, acc = pow(ipsi, 2 * j, q), pow(ipsi, j, q), 0     # psi^-((2i+1) j) = psi^-j (psi^-2j)^i
        for v in vals:
            acc += v * p
            p = p * step % q
        out.append(acc % q * ninv % q)
    return out


def _schoolbook(a, b, n, q):
    c = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                c[i + j] += x * y
            else:
                c[i + j - n] -= x * y
    return [v % q for v in c]


def _polys(words, n, q, psi):
    return [_inverse_by_definition(words[p * n:(p + 1) * n], n, q, psi) for p in range(words.size // n)]


@pytest.fixture(scope="module", params=[(6, 50), (6, 60), (8, 50), (8, 60)], ids=lambda p: "N%d-%dbit" % p)
def modulus(request, oracle):
    m, bits = request.param
    n = 1 << m
    q = oracle.find_prime(bits, n)
    psi = oracle.min_root(q, n)
    assert pow(psi, n, q) == q - 1, "psi is a primitive 2N-th root of unity"
    return n, q, psi, oracle.ctx(n, q, psi)


@pytest.mark.parametrize("lazy,bcast", [(False, False), (True, True)], ids=["canonical", "lazy-bcast"])
def test_dot_reference_is_the_sum_of_schoolbook_products(oracle, modulus, lazy, bcast):
    n, q, psi, cx = modulus
    aw, bw, want = kernel_recipes.dot_reference(oracle, cx, n, q, BATCH, 0, K, lazy, bcast)
    assert len(aw) == len(bw) == K
    if lazy:
        assert int(aw[0][kernel_recipes.W_LAZY]) == 4 * q - 1 and max(int(x.max()) for x in aw + bw) < 4 * q
    a = [_polys(x, n, q, psi) for x in aw]
    b = [_polys(x, n, q, psi) for x in bw]
    for p in range(BATCH):
        c = [0] * n
        for i in range(K):
            t = _schoolbook(a[i][p], b[i][0 if bcast else p], n, q)
            c = [(x + y) % q for x, y in zip(c, t)]
        assert [int(v) for v in want[p * n:(p + 1) * n]] == c, "polynomial %d" % p


@pytest.mark.parametrize("lazy,bcast,acc", [(False, False, False), (True, True, True)], ids=["store", "acc-lazy-bcast"])
def test_inverse_of_the_mul_reference_is_the_schoolbook_product(oracle, modulus, lazy, bcast, acc):
    n, q, psi, cx = modulus
    a, bw, c0, want = kernel_recipes.mul_reference(oracle, cx, n, q, BATCH, 0, lazy, bcast, acc)
    assert int(want[kernel_recipes.W_CARRY]) == (q - 2 if acc else q - 1)
    b = _polys(bw, n, q, psi)
    got = _polys(want, n, q, psi)
    before = _polys(c0, n, q, psi) if acc else None
    for p in range(BATCH):
        c = _schoolbook([int(v) for v in a[p * n:(p + 1) * n]], b[0 if bcast else p], n, q)
        if acc:
            c = [(x + y) % q for x, y in zip(c, before[p])]
        assert got[p] == c, "polynomial %d" % p
