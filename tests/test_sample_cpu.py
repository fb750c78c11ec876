"""CPU: the device-side sampler (ntt_rns_sample_batch) without a GPU -- the published Philox4x32-10 known answers and the recorded
anchors on the Python model of tests/sample_model.py, the statement functions of csrc/ntt_sample.h under the address and
undefined-behaviour sanitizers against that model (tests/sample_host_check.cpp, a stand-alone program), the distributions of the three
kinds on a fixed seed, the exported symbols, the constants and the option, the header as C and C++, the plain-C example against the
public header alone and the kernels of the new translation units: exactly the expected instances, none spilling or using scratch."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import children
import rns_support as rs
import sample_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd")
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libntt_mi355x.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
SYMBOLS = {"ntt_rns_sample_batch", "ntt_rns_sample_batch_strided"}
SEED = 0x5EED


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


# ---------------------------------------------------------------- the generator and the anchors

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert _hex(sm.philox(*counter, *key)) == want


def test_anchors_of_the_definition():
    assert sm.small(sm.TERNARY, SEED, 0, 8).tolist() == [0, 0, 0, -1, 0, -1, 0, 0]
    assert sm.small(sm.CBD21, SEED, 0, 8).tolist() == [-6, 6, -2, -2, 0, -2, 1, 6]
    assert [int(w) for w in sm.uniform(SEED, 0, 2, 3, (1 << 50) - 27)] == [0x3c27ecdd9b561, 0x40fadd3d78a]
    assert _hex(w[7] for w in sm.blocks(SEED, (1 << 32) + 5, 8, 1)) == "b33757ac 0e4e44e5 1b28e185 d0703e46"
    # the counter's words: s, P low, P high, tag; the key's: seed low, seed high
    assert _hex(w[0] for w in sm.blocks((7 << 32) | 9, (5 << 32) | 3, 12, sm.tag_of(sm.UNIFORM, 6))[:1]) == \
        _hex(sm.philox(0, 3, 5, 2 | (6 << 8), 9, 7)[:1])
    assert sm.tag_of(sm.TERNARY, 9) == 0 and sm.tag_of(sm.CBD21, 9) == 1 and sm.tag_of(sm.UNIFORM, 17) == 2 | (17 << 8)


def test_sample_uses_one_small_value_for_every_limb_and_a_tag_per_limb():
    primes = [(1 << 50) - 27, (1 << 30) - 35, 97]
    for kind in (sm.TERNARY, sm.CBD21):
        out = sm.sample(kind, primes, 64, 2, SEED, first_poly=(1 << 64) - 1, mult=5)
        v = np.concatenate([sm.small(kind, SEED, (1 << 64) - 1, 64), sm.small(kind, SEED, 0, 64)])  # P wraps mod 2^64
        for c, q in zip(out, primes):
            assert [int(x) for x in c] == [(5 * int(x)) % q for x in v]
    u = sm.sample(sm.UNIFORM, [97, 97], 64, 1, SEED)
    assert not np.array_equal(u[0], u[1]) and int(max(u[0].max(), u[1].max())) < 97


# ---------------------------------------------------------------- the distributions (deterministic: one seed)

COUNT = 4 << 14


def _small(kind):
    return np.concatenate([sm.small(kind, SEED, p, 1 << 14) for p in range(4)])


def test_ternary_distribution():
    """counts of -1 / 0 / 1 within 4 standard errors of n / 3 (sqrt(n (1/3) (2/3)) = 120.7)"""
    v = _small(sm.TERNARY)
    counts = [int(np.sum(v == x)) for x in (-1, 0, 1)]
    print("ternary counts", counts)
    assert sum(counts) == COUNT
    se = (COUNT * 2.0 / 9.0) ** 0.5
    for c in counts:
        assert abs(c - COUNT / 3.0) < 4 * se, counts


def test_cbd21_distribution():
    """mean 0 within 4 standard errors sqrt(10.5 / n) = 0.0127; variance 10.5 within 4 standard errors: a sum of independent
    symmetric two-point differences has negative excess kurtosis, its fourth central moment is below 3 sigma^4, so the sample variance's
    standard error is below sigma^2 sqrt(2 / n) = 0.058; |v| <= 21, and values beyond +-8 (2.5 sigma) occur among 65536 draws"""
    v = _small(sm.CBD21).astype(np.float64)
    mean, var = float(v.mean()), float(v.var())
    print("cbd21 mean %.4f variance %.3f extremes %d %d" % (mean, var, v.min(), v.max()))
    assert abs(mean) < 4 * (10.5 / COUNT) ** 0.5
    assert abs(var - 10.5) < 4 * 10.5 * (2.0 / COUNT) ** 0.5
    assert v.min() >= -21 and v.max() <= 21 and v.min() < -8 and v.max() > 8


def test_uniform_distribution():
    """mean of c / q within 4 standard errors sqrt(1 / (12 n)) = 0.0011 of 1/2 for a 50-bit prime; every word canonical; no word
    drawn twice (65536 draws from 2^50 values: a repeat has probability 2^-19)"""
    q = (1 << 50) - 27
    c = np.concatenate([sm.uniform(SEED, p, 1 << 14, 0, q) for p in range(4)])
    mean = float((c.astype(np.float64) / q).mean())
    print("uniform mean over q %.4f" % mean)
    assert int(c.max()) < q
    assert abs(mean - 0.5) < 4 * (1.0 / (12.0 * COUNT)) ** 0.5
    assert len(np.unique(c)) == COUNT
    # limb 3 (the anchor's tag), polynomial 0 alone: 2^14 words, standard error sqrt(1 / (12 * 2^14)) = 0.0023
    one = float((sm.uniform(SEED, 0, 1 << 14, 3, q).astype(np.float64) / q).mean())
    print("uniform mean over q, limb 3, polynomial 0: %.4f" % one)
    assert abs(one - 0.5) < 4 * (1.0 / (12.0 * (1 << 14))) ** 0.5


# ---------------------------------------------------------------- the host side of csrc/ntt_sample.h

@pytest.fixture(scope="module")
def host_check():
    return children.build_host_check("sample_host_check")


P_CORNERS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 63) + 7, (1 << 64) - 1]


def _positions():
    rng = np.random.default_rng(23)
    pairs = [(P, s) for P in P_CORNERS for s in (0, 1, 7, (1 << 14) - 1, (1 << 30) - 1)]
    pairs += [(int(P), int(s)) for P, s in zip(rng.integers(0, 1 << 63, size=200), rng.integers(0, 1 << 17, size=200))]
    return pairs


HOST_CASES = [(k, m) for k in (sm.TERNARY, sm.CBD21) for m in sm.MULTS] + [(sm.UNIFORM, 1)]  # (the uniform kind takes mult = 1)


@pytest.mark.parametrize("kind,mult", HOST_CASES, ids=["%s-mult%d" % (sm.KIND_IDS[k], i % 3) for i, (k, m) in enumerate(HOST_CASES)])
def test_host_statement_equals_the_model(lib, host_check, tmp_path, kind, mult):
    """sample_block, sample_small, sample_small_digit and sample_uniform_digit, compiled for the host with the sanitizers: 30-, 50- and
    60-bit primes, the multipliers 1, 65537 and 2^61 - 1 (the uniform kind: 1), positions with the P corners 2^32 - 1, 2^32 and 2^64 - 1
    -- word for word the model; the program itself compares the uniform word with the compiler's 128-bit division"""
    primes, _ = rs.chain(lib, 16, [30, 50, 60, 60])
    pairs = _positions()
    path = os.path.join(str(tmp_path), "vec.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n" % (kind, len(primes), mult, SEED << 20 | 5, len(pairs), " ".join(map(str, primes))))
        f.write("\n".join("%d %d" % p for p in pairs) + "\n")
    r = subprocess.run([host_check, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()], dtype=object)
    assert rows.shape == (len(pairs), 5 + len(primes))
    Ps, ss = [p[0] for p in pairs], [p[1] for p in pairs]
    seed = SEED << 20 | 5
    blk = sm.blocks_at(seed, Ps, ss, sm.tag_of(kind, 0))
    for i in range(4):
        assert [int(x) for x in rows[:, i]] == [int(x) for x in blk[i]], "block word %d" % i
    if kind == sm.UNIFORM:
        for l, q in enumerate(primes):
            want = sm.uniform_of(*sm.blocks_at(seed, Ps, ss, sm.tag_of(kind, l)), q)
            assert [int(x) for x in rows[:, 5 + l]] == [int(x) for x in want], l
        return
    v = sm.small_of(kind, blk[0], blk[1])
    assert [int(x) for x in rows[:, 4]] == v.tolist()
    for l, q in enumerate(primes):
        assert [int(x) for x in rows[:, 5 + l]] == [int(x) for x in sm.small_table(mult, q)[v + 21]], l


# ---------------------------------------------------------------- build checks

def test_exports_the_two_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOLS <= names, SYMBOLS - names
    assert SYMBOLS <= set(lib.EXPORTED_SYMBOLS)
    assert callable(lib.rns_sample)


def test_header_declares_the_constants_and_the_option_as_c_and_cxx(lib):
    header = open(os.path.join(ROOT, "include", "ntt_mi355x.h")).read()
    for name, val, mine in (("NTT_SAMPLE_TERNARY", 0, lib.SAMPLE_TERNARY), ("NTT_SAMPLE_CBD21", 1, lib.SAMPLE_CBD21),
                            ("NTT_SAMPLE_UNIFORM", 2, lib.SAMPLE_UNIFORM), ("NTT_SAMPLE_TRANSFORMED", 2, lib.SAMPLE_TRANSFORMED),
                            ("NTT_SAMPLE_ACCUMULATE", 4, lib.SAMPLE_ACCUMULATE), ("NTT_OPT_SAMPLE_FUSED", 24, lib.OPT_SAMPLE_FUSED)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), header) and mine == val, name
    assert (sm.TERNARY, sm.CBD21, sm.UNIFORM, sm.TRANSFORMED, sm.ACCUMULATE) == (0, 1, 2, 2, 4)
    assert (lib.SAMPLE_TRANSFORMED, lib.SAMPLE_ACCUMULATE) == (lib.LIFT_TRANSFORMED, lib.LIFT_ACCUMULATE)
    assert "not a cryptographic" in open(os.path.join(CSRC, "ntt_sample.h")).read().lower().replace("\n * ", " ")
    src = ('#include "ntt_mi355x.h"\nint main(void){return (NTT_SAMPLE_TERNARY == 0 && NTT_SAMPLE_CBD21 == 1 && NTT_SAMPLE_UNIFORM == 2 && '
           "NTT_SAMPLE_TRANSFORMED == 2 && NTT_SAMPLE_ACCUMULATE == 4 && NTT_OPT_SAMPLE_FUSED == 24 && ntt_rns_sample_batch && "
           "ntt_rns_sample_batch_strided) ? 0 : 1;}\n")
    children.syntax_check(src)


def test_example_builds_against_the_public_header(lib):
    assert os.path.exists(children.build_example(lib, "rns_sample", *children.STRICT))


def expected_instances():
    return rs.kernel_names("sample_fwd_kernel", rs.fused_launch_cases()) | {"sample_coef_kernel"}


def sample_kernels():
    """{normalised name: metadata} of every kernel in the sampling translation units (or, where the objects are not at hand, the
    sampling kernels of the linked library)"""
    import check_spills
    import kernel_inventory
    objs = sorted(glob.glob(os.path.join(CSRC, "sample*.o")))
    ks = [k for o in objs for k in check_spills.kernels_of(o)] if objs else \
        [k for k in check_spills.kernels_of(LIB) if "sample_" in k["name"]]
    names = [k["name"] for k in ks]
    return {kernel_inventory.normalise(d): k for d, k in zip(kernel_inventory.demangle(names), ks)}


def test_sample_objects_hold_exactly_the_expected_instances_without_spills():
    ks = sample_kernels()
    want = expected_instances()
    assert len(want) == 37
    assert set(ks) == want, ("missing %s, unexpected %s" % (sorted(want - set(ks))[:8], sorted(set(ks) - want)[:8]))
    bad = {n: (k.get("vgpr_spill_count"), k.get("sgpr_spill_count"), k.get("private_segment_fixed_size"))
           for n, k in ks.items()
           if k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)}
    assert not bad, "spills / scratch: %s" % bad
