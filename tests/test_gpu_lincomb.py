"""GPU: ntt_rns_lincomb_batch -- c (+)= bias + sum_i sigma_{g_i}(a_i) * mu_i per limb and word.  Every output word is compared with the
model of tests/lincomb_model.py (the definition in Python integers; through the oracle's modular product for the large shapes),
exactly; the operands sit among canaries, which stay untouched, as the inputs do."""
import os

import numpy as np
import pytest

import children
import galois_model as gm
import lincomb_model as lm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "lincomb_model.py")
A, B, LZ = lm.ACCUMULATE, lm.M_BROADCAST, lm.LAZY_IN


def _gs(n, k=5):
    """k Galois elements out of {1, 5, 25, 2N - 1, 5^-1 mod 2N} (reduced mod 2N), in turn"""
    base = [1, 5 % (2 * n), 25 % (2 * n), 2 * n - 1, pow(5, -1, 2 * n)]
    return [base[i % 5] for i in range(k)]


# ---------------------------------------------------------------- shapes

@pytest.mark.gpu
@pytest.mark.parametrize("nlimbs", [1, 17])
@pytest.mark.parametrize("batch", [1, 3, 130])
@pytest.mark.parametrize("logn", [1, 6, 12])
def test_shapes(lib, oracle, logn, batch, nlimbs):
    """k = 3: a scalar term, a term with a polynomial multiplier read through sigma_5, a scalar term through the conjugation; a
    different scalar per term and limb and a different bias per limb (17 limbs: two launches -- a wrong limb index shows)"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [60] + [50] * (nlimbs - 1))
    lm.run_case(lib, oracle, primes, roots, n, batch, [1, 5 % (2 * n), 2 * n - 1], poly=(1,), seed=logn + batch)


@pytest.mark.gpu
def test_grid_wrap(lib, oracle):
    """NTT_OPT_MAX_GRID = 3 on plans[0] at 2^10, 5 polynomials: every thread walks several iterations and polynomials"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, [50, 50])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    plans[0].set_option(lib.OPT_MAX_GRID, 3)
    lm.run_case(lib, oracle, primes, roots, n, 5, _gs(n, 3), poly=(0, 2), flags=A, plans=plans, seed=4)
    for p in plans:
        p.destroy()


# ---------------------------------------------------------------- term counts, Galois elements

@pytest.mark.gpu
@pytest.mark.parametrize("mix", ["scalars_null_m", "scalars", "every_third_poly", "all_poly"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 16])
def test_term_counts(lib, oracle, k, mix):
    """the load groups of four and their tail; scalar and polynomial terms in one call (d_m NULL, NULL entries inside d_m)"""
    n = 64
    primes, roots = rs.chain(lib, n, [60, 30])
    poly = {"scalars_null_m": (), "scalars": (), "every_third_poly": tuple(range(0, k, 3)), "all_poly": tuple(range(k))}[mix]
    lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, k), poly=poly, null_m=mix == "scalars_null_m", seed=k)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [1, 2, 6, 12])
def test_a_galois_element_per_term(lib, oracle, logn):
    """k = 5, g_i = 1, 5, 25, 2N - 1, 5^-1 mod 2N in one call (N = 2 and 4: what they reduce to), scalars and multipliers mixed"""
    n = 1 << logn
    primes, roots = rs.chain(lib, n, [60, 50, 30])
    lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n), poly=(1, 4), flags=A, seed=logn)
    lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n)[::-1], poly=(0,), flags=B, seed=logn + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [1, 2, 10])
def test_one_unit_term_is_the_automorphism_word_for_word(lib, oracle, logn):
    """k = 1, scalar 1 (h_s NULL), no bias: ntt_rns_galois_batch's output"""
    n, batch = 1 << logn, 3
    primes, roots = rs.chain(lib, n, [60, 50, 52])
    for g in sorted(set(_gs(n))):
        got = lm.run_case(lib, oracle, primes, roots, n, batch, [g], scalars=None, bias=None, seed=3)
        a = [oracle.fill_uniform(batch * n, q, 3 * 1000 + l) for l, q in enumerate(primes)]
        for l, q in enumerate(primes):
            edge = [0, q - 1, (q - 1) // 2, (q + 1) // 2][:min(4, n)]
            a[l][:len(edge)] = edge
        want = gm.run_galois(lib, oracle, primes, roots, n, batch, g, gm.TRANSFORMED, limbs=a)
        for l in range(len(primes)):
            assert np.array_equal(got[l], want[l]), (g, l)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, A, B, A | B])
def test_equal_g_and_multipliers_is_the_rotation_key_product_word_for_word(lib, oracle, flags):
    """every g_i equal, every term with a polynomial multiplier: ntt_rns_galois_dot_batch's output on the same operands"""
    n, batch, k = 1 << 8, 3, 5
    primes, roots = rs.chain(lib, n, [60, 50])
    g = pow(5, 3, 2 * n)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    a = [[oracle.fill_uniform(batch * n, q, 50 * i + l) for l, q in enumerate(primes)] for i in range(k)]
    m = [[oracle.fill_uniform(n if flags & B else batch * n, q, 50 * i + 7 + l) for l, q in enumerate(primes)] for i in range(k)]
    c0 = [oracle.fill_uniform(batch * n, q, 999 + l) for l, q in enumerate(primes)]
    bufs = [lib.DeviceBuffer(x[0].size * 2).upload(np.concatenate(x)) for x in a + m]
    outs = [lib.DeviceBuffer(2 * batch * n).upload(np.concatenate(c0)) for _ in range(2)]
    ap, mp = [b.ptr for b in bufs[:k]], [b.ptr for b in bufs[k:]]
    lib.rns_lincomb(plans, outs[0].ptr, ap, mp, None, [g] * k, None, batch, flags)
    lib.rns_galois_dot(plans, outs[1].ptr, ap, mp, g, batch,
                       gm.TRANSFORMED | (gm.ACCUMULATE if flags & A else 0) | (gm.KEY_BROADCAST if flags & B else 0))
    got, want = outs[0].download(), outs[1].download()
    for b in bufs + outs:
        b.free()
    for p in plans:
        p.destroy()
    assert np.array_equal(got, want)
    ref = lm.model(primes, c0, a, m, [[0] * 2] * k, [g] * k, [0, 0], n, flags)
    assert np.array_equal(got, np.concatenate(ref))


# ---------------------------------------------------------------- mixed chain, extremes, flags

CHAIN = [60, 50, 30, 52]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["zero", "top", "k16_top_accumulate", "lazy_top_k8", "lazy_random_k8", "k9_lazy_refused"])
def test_mixed_chain_and_extremes(lib, oracle, case):
    n = 64
    primes, roots = rs.chain(lib, n, CHAIN)
    top = [[q - 1 for q in primes]] * 16
    if case == "zero":
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 4), poly=(1,), flags=A, fill=lambda q: 0, scalars=[[0] * 4] * 4, bias=[0] * 4)
    elif case == "top":
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 4), poly=(1,), fill=lambda q: q - 1, scalars=top[:4], bias=top[0])
    elif case == "k16_top_accumulate":
        # the bound of the header: 16 (q - 1)^2 + (q - 1) + (q - 1), on scalars and on polynomial multipliers
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 16), flags=A, fill=lambda q: q - 1, scalars=top, bias=top[0])
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 16), poly=tuple(range(16)), flags=A, fill=lambda q: q - 1, bias=top[0])
    elif case == "lazy_top_k8":
        # every a word 4q - 1, every multiplier, c and the bias q - 1: the 60-bit and the 30-bit limb among the four
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 8), flags=A | LZ, fill=lambda q: q - 1, scalars=top[:8], bias=top[0])
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 8), poly=tuple(range(8)), flags=A | LZ, fill=lambda q: q - 1, bias=top[0])
    elif case == "lazy_random_k8":
        lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 8), poly=(2, 5), flags=LZ, seed=8)
    else:
        with pytest.raises(lib.NttError, match="1 .. 8"):
            lm.run_case(lib, oracle, primes, roots, n, 3, _gs(n, 9), flags=LZ)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, A, B, A | B])
def test_flags(lib, oracle, flags):
    n = 1 << 7
    primes, roots = rs.chain(lib, n, CHAIN)
    lm.run_case(lib, oracle, primes, roots, n, 5, _gs(n, 4), poly=(0, 3), flags=flags, seed=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, A])
def test_bias_with_one_term(lib, oracle, flags):
    """k = 1, h_s NULL: c (+)= a + bias_l"""
    n = 1 << 7
    primes, roots = rs.chain(lib, n, CHAIN)
    lm.run_case(lib, oracle, primes, roots, n, 2, [1], scalars=None, flags=flags, seed=6)


@pytest.mark.gpu
def test_add_sub_neg(lib, oracle):
    """the convenience calls, in place and out of place"""
    n, batch = 1 << 6, 3
    primes, roots = rs.chain(lib, n, CHAIN)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    a = [oracle.fill_uniform(batch * n, q, l) for l, q in enumerate(primes)]
    b = [oracle.fill_uniform(batch * n, q, 10 + l) for l, q in enumerate(primes)]
    da, db = (lib.DeviceBuffer(4 * batch * n).upload(np.concatenate(x)) for x in (a, b))
    dc = lib.DeviceBuffer(4 * batch * n)
    qs = np.concatenate([np.full(batch * n, q, dtype=np.uint64) for q in primes])
    A_, B_ = np.concatenate(a), np.concatenate(b)
    lib.rns_add(plans, dc.ptr, da.ptr, db.ptr, batch)
    assert np.array_equal(dc.download(), (A_ + B_) % qs)
    lib.rns_sub(plans, dc.ptr, da.ptr, db.ptr, batch)
    assert np.array_equal(dc.download(), (A_ + qs - B_) % qs)
    lib.rns_neg(plans, dc.ptr, da.ptr, batch)
    assert np.array_equal(dc.download(), (qs - A_) % qs)
    lib.rns_sub(plans, db.ptr, da.ptr, db.ptr, batch)  # b = a - b in place
    assert np.array_equal(db.download(), (A_ + qs - B_) % qs)
    lib.rns_neg(plans, da.ptr, da.ptr, batch)
    assert np.array_equal(da.download(), (qs - A_) % qs)
    for x in (da, db, dc):
        x.free()
    for p in plans:
        p.destroy()


# ---------------------------------------------------------------- aliasing, layouts

@pytest.mark.gpu
@pytest.mark.parametrize("alias", [("a", 0), ("m", 1)], ids=["c_is_a0", "c_is_m1"])
def test_in_place_equals_out_of_place(lib, oracle, alias):
    """c == a_0 (g_0 = 1) and c == m_1: the result of the out-of-place call on the same operands"""
    n = 1 << 10
    primes, roots = rs.chain(lib, n, CHAIN)
    gs = [1, 5, 2 * n - 1]
    out = lm.run_case(lib, oracle, primes, roots, n, 3, gs, poly=(1, 2), seed=12)
    inp = lm.run_case(lib, oracle, primes, roots, n, 3, gs, poly=(1, 2), seed=12, alias=alias)
    for l in range(len(primes)):
        assert np.array_equal(inp[l], out[l]), l


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["limb", "batch", "batch_padded", "limb_padded", "odd_limb_stride"])
@pytest.mark.parametrize("flags", [A, B])
def test_layouts(lib, oracle, layout, flags):
    """[limb][batch][N], [batch][limb][N], padded strides, an odd limb stride; 17 limbs: the second launch's offsets too"""
    n, batch, nl = 1 << 6, 3, 17
    primes, roots = rs.chain(lib, n, [60] + [50] * (nl - 1))
    if layout == "odd_limb_stride":
        ls, ps = n + 1, nl * (n + 1) + 3
        layout = (ls, ps, (batch - 1) * ps + (nl - 1) * ls + n + 5)
    lm.run_case(lib, oracle, primes, roots, n, batch, _gs(n, 3), poly=(1,), flags=flags, layout=layout, seed=2)


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_argument_errors_write_nothing(lib, oracle):
    n, batch = 1 << 8, 2
    primes, roots = rs.chain(lib, n, [50] * 3)
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    q2 = lib.find_prime(50, 2 * n)
    other = lib.Plan(2 * n, q2, lib.min_root(q2, 2 * n))
    span = 3 * batch * n
    pat = oracle.fill_uniform(20 * span, primes[0], 5)
    buf = lib.DeviceBuffer(20 * span).upload(pat)
    o = [buf.ptr + 8 * i * span for i in range(20)]  # twenty disjoint three-limb operands inside the buffer
    c, a = o[0], o[1:18]

    def refused(what, message, ps=plans, c=c, das=a[:2], dms=None, scalars=None, gs=None, bias=None, flags=0, lay=None):
        with pytest.raises(lib.NttError, match="status -1"):
            lib.rns_lincomb(ps, c, das, dms, scalars, gs, bias, batch, flags, layout=lay)
        assert message in lib.last_error(), (what, lib.last_error())
        assert np.array_equal(buf.download(), pat), what

    ones = [1] * 3
    refused("no limb", "limb list", ps=[])
    refused("no term", "1 .. 16", das=[])
    refused("17 terms", "1 .. 16", das=a[:17])
    refused("9 lazy terms", "1 .. 8", das=a[:9], flags=LZ)
    refused("null c", "null", c=None)
    refused("null a_1", "null", das=[a[0], None])
    refused("even g", "odd", gs=[1, 4])
    refused("g = 0", "odd", gs=[1, 0])
    refused("g = 2N + 1", "below 2N", gs=[1, 2 * n + 1])
    refused("a scalar equal to q", "scalar", scalars=[ones, [1, primes[1], 1]])
    refused("a bias equal to q", "bias", bias=[0, 0, primes[2]])
    refused("differing N", "share N", ps=[plans[0], other, plans[2]])
    refused("unknown flag", "unknown flag", flags=8)
    refused("broadcast without a multiplier", "M_BROADCAST", flags=B)
    refused("broadcast with only NULL entries", "M_BROADCAST", dms=[None, None], flags=B)
    refused("overlapping strides", "overlap", lay=(n, n))
    refused("c is an a_i with g != 1", "g is not 1", das=[a[0], c], gs=[1, 5])
    refused("c inside a_0", "overlaps an a_i", c=a[0] + 8 * n)
    refused("c overlapping a_1's tail", "overlaps an a_i", c=a[1] + 8 * (span - n))
    refused("c shifted against a multiplier", "multiplier", dms=[None, c + 8])
    refused("c is a broadcast multiplier", "multiplier", dms=[None, c], flags=B)
    # what is read only where it is used: the scalars of a term with a polynomial multiplier are not checked
    lib.rns_lincomb(plans, c, a[:2], [a[2], None], [[primes[0]] * 3, ones], None, None, batch, 0)
    assert not np.array_equal(buf.download()[:span], pat[:span]) and np.array_equal(buf.download()[span:], pat[span:])
    for p in plans + [other]:
        p.destroy()
    buf.free()


# ---------------------------------------------------------------- graph capture, launches, the example

@pytest.mark.gpu
def test_captured_in_a_hip_graph():
    """one accumulating call (2^10, 17 limbs: two launches, k = 3 with a polynomial multiplier and three Galois elements) captured into
    a HIP graph and replayed twice: the model applied twice (a process of its own: torch has to be imported before the library).  The
    host arrays are released before the replay: the launch carries its own copy."""
    code = """
import torch
torch.cuda.set_device(0)
import numpy as np
import ontt
from oracle_binding import Oracle
import lincomb_model as lm
import rns_support as rs
lib, orc = ontt.load(), Oracle()
n, batch, k = 1 << 10, 3, 3
primes, roots = rs.chain(lib, n, [60] + [50] * 16)
nl = len(primes)
plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
gs = [1, 5, 2 * n - 1]
scalars, bias = lm.distinct_scalars(primes, k, 1)
a = [[orc.fill_uniform(batch * n, q, 100 * i + l) for l, q in enumerate(primes)] for i in range(k)]
m = [None, [orc.fill_uniform(batch * n, q, 77 + l) for l, q in enumerate(primes)], None]
c0 = [orc.fill_uniform(batch * n, q, 55 + l) for l, q in enumerate(primes)]
dev = lambda x: torch.from_numpy(np.concatenate(x).view(np.int64)).to("cuda:0")
da, dm, dc = [dev(x) for x in a], dev(m[1]), dev(c0)
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=0)
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.graph(g, stream=s):
    st = torch.cuda.current_stream().cuda_stream
    lib.rns_lincomb(plans, dc.data_ptr(), [x.data_ptr() for x in da], [None, dm.data_ptr(), None], [list(r) for r in scalars], list(gs),
                    list(bias), batch, lm.ACCUMULATE, stream=st)
want = c0
for rep in (1, 2):
    g.replay()
    torch.cuda.synchronize()
    want = lm.model(primes, want, a, m, scalars, gs, bias, n, lm.ACCUMULATE)
    got = dc.cpu().numpy().view(np.uint64).reshape(nl, batch * n)
    for l in range(nl):
        assert np.array_equal(got[l], want[l]), (rep, l)
print("graph ok")
"""
    children.python_child(code, 300)


@pytest.mark.gpu
def test_route_proof_one_launch_per_16_limbs():
    """one traced process: the call over 16 limbs launches lincomb_kernel once, the call over 17 limbs twice, and neither anything
    else (the calls are told apart by the table kernels of the plans each creates first)"""
    launched = children.traced(MODEL_PY, ["--route"], 300)
    calls, setup = [], True
    for k in launched:
        if k.split("<")[0] in rs.SETUP_KERNELS:
            setup = True
            continue
        if setup:
            calls.append([])
        setup = False
        calls[-1].append(k)
    assert calls == [["lincomb_kernel"], ["lincomb_kernel"] * 2], launched


@pytest.mark.gpu
def test_example_prints_ok_for_every_limb(lib):
    out = children.run_example(lib, "rns_lincomb")
    lines = [line for line in out.splitlines() if line.startswith("limb ")]
    assert len(lines) == 8 and all(line.endswith(" OK") for line in lines), out
