"""CPU: the lifts into the RNS (ntt_rns_from_plain_batch, ntt_rns_from_double_batch) without a GPU -- the statement functions of
csrc/ntt_lift.h under the address and undefined-behaviour sanitizers against the three big-integer definitions of tests/lift_model.py
(tests/lift_host_check.cpp, a stand-alone program), the [Delta]_q identity of the host constants, the exported symbols, the flags and
the option, the header as C and C++, the plain-C example against the public header alone and the kernels of the new translation
units: exactly the expected instances, none spilling or using scratch."""
import glob
import os
import random
import re
import subprocess
import sys
from math import prod

import numpy as np
import pytest

import children
import lift_model as lm
import rns_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd")
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
SYMBOLS = {"ntt_rns_from_plain_batch", "ntt_rns_from_plain_batch_strided", "ntt_rns_from_double_batch", "ntt_rns_from_double_batch_strided"}
CHAINS = {"L1_30": [30], "L1_60": [60], "L3_50": [50] * 3, "L3_mixed": [60, 30, 52], "L16_60": [60] * 16, "L16_30": [30] * 16}


# ---------------------------------------------------------------- the definitions themselves

def test_definitions_on_small_numbers():
    assert [lm.centred(m, 5) for m in range(5)] == [0, 1, 2, -2, -1] and [lm.centred(m, 4) for m in range(4)] == [0, 1, -2, -1]
    assert [lm.scaled(m, 4, 10) for m in range(4)] == [0, 3, 5, 8]  # 2.5 -> 3 (ties up), 5, 7.5 -> 8
    bits = lambda v: int(np.float64(v).view(np.uint64))
    assert [lm.rounded(bits(v), 1.0) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 2.0 ** 127, float("nan"), float("-inf"), 5e-324)] == [0, 2, 2, 0, -2, 0, 0, 0, 0]
    assert lm.rounded(bits(np.nextafter(2.0 ** 127, 0)), 1.0) == 2 ** 127 - 2 ** 74 and lm.rounded(bits(2.0 ** 126), 2.0) == 0
    assert lm.rounded(bits(1.0 / 3.0), 3.0) == 1 and lm.rounded(bits(2.0 ** 53 + 2), 1.0) == 2 ** 53 + 2


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_delta_identity_of_the_host_constants(lib, chain):
    """floor((Q m + floor(t/2)) / t) = Delta m + floor((r m + floor(t/2)) / t) with Delta = floor(Q / t), r = Q mod t, and
    [Delta]_q = -r t^-1 mod q for every prime coprime to t: what host_lift.inc and lift_scaled compute, against the definition, the ties
    of even t included"""
    primes, _ = rs.chain(lib, 16, CHAINS[chain])
    Q = prod(primes)
    rng = random.Random(len(primes))
    for t in lm.TS:
        if any(t % q == 0 for q in primes):
            continue
        r, delta = Q % t, Q // t
        for q in primes:
            assert delta % q == (-r * pow(t, -1, q)) % q
        for m in lm.plain_corners(t, primes) + [rng.randrange(t) for _ in range(50)]:
            w = (r * m + t // 2) // t
            assert 0 <= w <= t and lm.scaled(m, t, Q) == delta * m + w


def test_corner_generator_builds_ties_and_boundaries(lib):
    primes, _ = rs.chain(lib, 16, [50] * 3)
    Q = prod(primes)
    for t in (256, 1 << 32, 65537, 10 ** 18 + 9):
        r = Q % t
        rests = {(r * m + t // 2) % t for m in lm.plain_corners(t, primes)}
        assert 0 in rests and t - 1 in rests, t  # at a multiple of t, and just below one
        if t % 2 == 0:
            assert any((r * m) % t == t // 2 for m in lm.plain_corners(t, primes)), t  # a tie: Q m / t = k + 1/2
        up = t - t // 2
        assert {0, 1, up - 1, up, t - 1} <= set(lm.plain_corners(t, primes))


# ---------------------------------------------------------------- the host side of csrc/ntt_lift.h

@pytest.fixture(scope="module")
def host_check():
    return children.build_host_check("lift_host_check")


def _run(host_check, tmp_path, mode, primes, t, scale, words):
    path = os.path.join(str(tmp_path), "vec.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n" % (mode, len(primes), t, int(np.float64(scale).view(np.uint64)), len(words)))
        f.write(" ".join(map(str, primes)) + "\n" + "\n".join(str(int(w)) for w in words) + "\n")
    r = subprocess.run([host_check, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    return [np.array(col, dtype=np.uint64) for col in zip(*rows)]


@pytest.mark.parametrize("mode", [lm.CENTRED, lm.SCALED])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_host_statement_equals_the_definition(lib, host_check, tmp_path, chain, mode):
    """lift_word and lift_digit, compiled for the host with the sanitizers, for every t: the corner words and random draws, word for
    word the big-integer definition; the program itself compares the 128-by-64-bit quotient with the compiler's division"""
    primes, _ = rs.chain(lib, 16, CHAINS[chain])
    rng = random.Random(len(primes) * 3 + (mode == lm.SCALED))
    for t in lm.TS:
        if mode == lm.SCALED and any(t % q == 0 for q in primes):
            continue
        words = lm.plain_corners(t, primes if mode == lm.SCALED else None) + [rng.randrange(t) for _ in range(120)]
        got = _run(host_check, tmp_path, 1 if mode == lm.SCALED else 0, primes, t, 0.0, words)
        want = lm.lift(mode, words, primes, t)
        for l, q in enumerate(primes):
            assert np.array_equal(got[l], want[l]), (t, l)
            assert int(got[l].max()) < q


def test_host_statement_stays_canonical_for_words_above_t(lib, host_check, tmp_path):
    """m >= t is the caller's error: the word is unspecified, but below q"""
    primes, _ = rs.chain(lib, 16, [60, 30, 50])
    words = [(1 << 64) - 1, 1 << 63, (1 << 61) + 5, 65537, 65538]
    for mode in (0, 1):
        for t in (2, 65537, (1 << 61) - 1):
            got = _run(host_check, tmp_path, mode, primes, t, 0.0, words)
            for l, q in enumerate(primes):
                assert int(got[l].max()) < q


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 40, 1.0 / 3.0, 3.0, 2.0 ** -1074, -7.5])
@pytest.mark.parametrize("chain", ["L1_30", "L3_mixed", "L16_60"])
def test_host_double_equals_the_definition(lib, host_check, tmp_path, chain, scale):
    primes, _ = rs.chain(lib, 16, CHAINS[chain])
    words = np.concatenate([lm.double_corners(), lm.random_plain(lm.DOUBLE, 200, 0, 5),
                            (np.random.default_rng(6).standard_normal(64) * 2.0 ** 120).view(np.uint64)])
    got = _run(host_check, tmp_path, 2, primes, 0, scale, words)
    want = lm.lift(lm.DOUBLE, words, primes, scale=scale)
    for l in range(len(primes)):
        assert np.array_equal(got[l], want[l]), l


# ---------------------------------------------------------------- build checks

def test_exports_the_four_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOLS <= names, SYMBOLS - names
    assert SYMBOLS <= set(lib.EXPORTED_SYMBOLS)
    assert callable(lib.rns_from_plain) and callable(lib.rns_from_double)


def test_header_declares_the_flags_and_the_option_as_c_and_cxx(lib):
    header = open(os.path.join(ROOT, "include", "ntt_mi355x.h")).read()
    for name, val, mine in (("NTT_LIFT_SCALE", 1, lib.LIFT_SCALE), ("NTT_LIFT_TRANSFORMED", 2, lib.LIFT_TRANSFORMED),
                            ("NTT_LIFT_ACCUMULATE", 4, lib.LIFT_ACCUMULATE), ("NTT_OPT_LIFT_FUSED", 22, lib.OPT_LIFT_FUSED)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), header) and mine == val, name
    assert (lm.SCALE, lm.TRANSFORMED, lm.ACCUMULATE) == (1, 2, 4)
    src = ('#include "ntt_mi355x.h"\nint main(void){return (NTT_LIFT_SCALE == 1 && NTT_LIFT_TRANSFORMED == 2 && NTT_LIFT_ACCUMULATE == 4 && '
           "NTT_OPT_LIFT_FUSED == 22 && ntt_rns_from_plain_batch && ntt_rns_from_plain_batch_strided && "
           "ntt_rns_from_double_batch && ntt_rns_from_double_batch_strided) ? 0 : 1;}\n")
    children.syntax_check(src)


def test_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_encrypt", *children.STRICT))


def expected_instances():
    return rs.kernel_names("lift_fwd_kernel", rs.fused_launch_cases()) | {"lift_coef_kernel"}


def lift_kernels():
    """{normalised name: metadata} of every kernel in the lift translation units (or, where the objects are not at hand, the lift
    kernels of the linked library)"""
    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "lift*.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if "lift_" in k["name"]]
    names = [k["name"] for k in ks]
    return {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}


def test_lift_objects_hold_exactly_the_expected_instances_without_spills():
    ks = lift_kernels()
    want = expected_instances()
    assert len(want) == 37
    assert set(ks) == want, ("missing %s, unexpected %s" % (sorted(want - set(ks))[:8], sorted(set(ks) - want)[:8]))
    bad = {n: (k.get("vgpr_spill_count"), k.get("sgpr_spill_count"), k.get("private_segment_fixed_size"))
           for n, k in ks.items()
           if k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)}
    assert not bad, "spills / scratch: %s" % bad
