#!/usr/bin/env python3
"""tools/modup_mul_bench.py [--quick] [--prev LIB] [--logn 13 14]: one digit's term of the key-switching inner product,
c^ += fwd(ModUp(digit)) (.) key^ (broadcast key, accumulating), timed with device events after warm-ups:

  fused    ntt_rns_mod_up_mul_batch, NTT_OPT_MODUP_FUSED 1 (modup_mul_kernel on every run)            -- this library
  comp     ntt_rns_mod_up_mul_batch, NTT_OPT_MODUP_FUSED 0 (the composition)                           -- this library
  auto     ntt_rns_mod_up_mul_batch, NTT_OPT_MODUP_FUSED -1 (the default rule)                         -- this library
  pair     ntt_rns_mod_up_batch + ntt_rns_fwd_mul_batch, the two calls                                 -- this library
  parent   ntt_rns_mod_up_batch + ntt_rns_fwd_mul_batch, the two calls a caller issues today           -- the PARENT commit's library
           (LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, 24 limbs of 50-bit primes (runs of 16 and 8), digit (0, count), count in {1, 2, 3, 4, 6, 8}, 2 / 64 / 1024
polynomials.  The two libraries run in ALTERNATING child processes on the same board, round by round; a child times every shape.
Inside a child the variants of a shape are timed INTERLEAVED, three windows each in an order that rotates from round to round (a
window timed straight behind the longest variant's is no longer always the same variant's), and a variant's figure for the round is
the median of its windows.  Printed per shape: the median ms per call of each variant, and the call-rate ratios parent / variant as
RANGES over the rounds (round r of one against round r of the other); the parent's own spread over the rounds (max / min); and
ntt_copy_probe of one operand (8 nl batch N bytes read, as many written) in the same child for scale.  `pair` separates the two
things `comp` differs from `parent` in: the library (parent / pair) and one call instead of two from the host (pair / comp); the
one-call variants set NTT_OPT_MODUP_FUSED inside every timed call (one more host call each).
Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer rounds and shapes (a smoke run of the tool)")
ap.add_argument("--prev", default=os.path.join(ROOT, "build", "libntt_prev.so"), help="the parent commit's library")
ap.add_argument("--logn", type=int, nargs="+", default=[13, 14])
ap.add_argument("--child", nargs=3, metavar=("WHICH", "LOGN", "ROUND"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (8, 10, 3, 3)
NL = 24
COUNTS = (1, 4) if a.quick else (1, 2, 3, 4, 6, 8)
BATCHES = (2, 64) if a.quick else (2, 64, 1024)
FLAGS = 2 | 4  # NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"count,batch,variant": ms per call} as one JSON line"""
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    plans = []
    for k in range(NL):
        q = lib.find_prime(50, n, k)
        plans.append(lib.Plan(n, q, lib.min_root(q, n)))
    top = max(BATCHES)
    dext, dc, dk = lib.DeviceBuffer(NL * top * n), lib.DeviceBuffer(NL * top * n), lib.DeviceBuffer(NL * n)
    for l, p in enumerate(plans):
        lib.fill_uniform(dk.ptr + 8 * l * n, n, p.q, 500 + l, 0)
    e0, e1 = lib.Event(), lib.Event()

    def window(fn):
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        lib.stream_sync()
        return e1.elapsed_ms_since(e0) / CALLS

    def interleaved(fns):
        """{name: median ms per call over WINDOWS windows}, the variants' windows alternating in an order rotated by the round"""
        names = sorted(fns)
        names = names[rnd % len(names):] + names[:rnd % len(names)]
        for name in names:
            for _ in range(WARM):
                fns[name]()
        lib.stream_sync()
        t = {name: [] for name in names}
        for _ in range(WINDOWS):
            for name in names:
                t[name].append(window(fns[name]))
        return {name: statistics.median(v) for name, v in t.items()}

    def pair_of(count, batch):
        def pair():
            lib.rns_mod_up(plans, dext.ptr, 0, count, batch, 0)
            lib.rns_fwd_mul(plans, dc.ptr, dext.ptr, dk.ptr, batch, FLAGS)
        return pair

    def one_call(opt, count, batch):
        def call():
            plans[0].set_option(lib.OPT_MODUP_FUSED, opt)
            lib.rns_mod_up_mul(plans, dc.ptr, dext.ptr, 0, count, dk.ptr, batch, FLAGS)
        return call

    out = {}
    for batch in BATCHES:
        per = batch * n
        for l, p in enumerate(plans):  # canonical words in every slot: c^ and the digit wherever it starts
            lib.fill_uniform(dext.ptr + 8 * l * per, per, p.q, 77 + l, 0)
            lib.fill_uniform(dc.ptr + 8 * l * per, per, p.q, 177 + l, 0)
        lib.stream_sync()
        out["0,%d,copy" % batch] = interleaved({"copy": lambda: lib.copy_probe(dc.ptr, dext.ptr, NL * per)})["copy"]
        for l, p in enumerate(plans):
            lib.fill_uniform(dc.ptr + 8 * l * per, per, p.q, 177 + l, 0)
        for count in COUNTS:
            if which == "prev":
                fns = {"parent": pair_of(count, batch)}
            else:
                fns = {"fused": one_call(1, count, batch), "comp": one_call(0, count, batch), "auto": one_call(-1, count, batch),
                       "pair": pair_of(count, batch)}
            for name, ms in interleaved(fns).items():
                out["%d,%d,%s" % (count, batch, name)] = ms
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/modup_mul_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# %d limbs of 50-bit primes, digit (0, count), broadcast key, accumulating; %d rounds of alternating child processes, each timing" % (NL, ROUNDS))
    print("# the variants of a shape interleaved, %d windows each, in an order rotated by the round" % WINDOWS)
    print("# %d calls after %d warm-up calls per shape; ms = median over the rounds; ratios = parent ms / variant ms, min..max over the rounds" % (CALLS, WARM))
    for logn in a.logn:
        rounds = {"prev": [], "cur": []}
        for rnd in range(ROUNDS):
            for which in ("prev", "cur"):
                env = dict(os.environ)
                if which == "prev":
                    env["NTT_LIB"] = a.prev
                else:
                    env.pop("NTT_LIB", None)
                args = [sys.executable, os.path.abspath(__file__), "--child", which, str(logn), str(rnd)] + (["--quick"] if a.quick else [])
                r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("child %s 2^%d failed (%d): %s" % (which, logn, r.returncode, r.stderr[-2000:]))
                rounds[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
        for batch in BATCHES:
            cp = [r["0,%d,copy" % batch] for r in rounds["cur"]]
            print("copy   N=2^%d polys=%-5d ntt_copy_probe of one operand (%.1f MB read + written) %8.4f ms" % (
                logn, batch, 16.0 * NL * batch * (1 << logn) / 1e6, statistics.median(cp)))
            for count in COUNTS:
                par = [r["%d,%d,parent" % (count, batch)] for r in rounds["prev"]]
                v = {name: [r["%d,%d,%s" % (count, batch, name)] for r in rounds["cur"]] for name in ("fused", "comp", "auto", "pair")}
                ratio = {name: [p / t for p, t in zip(par, ts)] for name, ts in v.items()}
                print("modup_mul N=2^%d polys=%-5d count=%d  parent pair %8.4f ms (spread %.2f)  fused %8.4f ms  comp %8.4f ms  auto %8.4f ms  "
                      "pair %8.4f ms  parent/fused %s  parent/comp %s  parent/auto %s  parent/pair %s" % (
                          logn, batch, count, statistics.median(par), max(par) / min(par), statistics.median(v["fused"]),
                          statistics.median(v["comp"]), statistics.median(v["auto"]), statistics.median(v["pair"]), rng(ratio["fused"]),
                          rng(ratio["comp"]), rng(ratio["auto"]), rng(ratio["pair"])))
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
