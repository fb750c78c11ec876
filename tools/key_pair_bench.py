#!/usr/bin/env python3
"""tools/key_pair_bench.py [--quick] [--prev LIB] [--logn 13 14]: one digit's term of BOTH components of a key switch,
c0^ += fwd(ModUp(digit)) (.) key0^, c1^ += fwd(ModUp(digit)) (.) key1^ (broadcast keys, accumulating), the pair form of the
forward-multiply (no conversion: printed as count 0) and the pair form of the rotation key product, timed with device events after
warm-ups:

  fused    the pair call, NTT_OPT_PAIR_FUSED 1 (modup_mul2_kernel on every run)                          -- this library
  comp     the pair call, NTT_OPT_PAIR_FUSED 0 (conversion, ONE transform, one two-output product)       -- this library
  auto     the pair call, NTT_OPT_PAIR_FUSED -1 (the default rule)                                       -- this library
  A        the single call twice (ntt_rns_mod_up_mul_batch / ntt_rns_fwd_mul_batch, its default route)   -- the PARENT commit's library
  B        ntt_rns_mod_up_batch (not for count 0) + ntt_rns_fwd_batch + two element-wise accumulates
           (ntt_rns_galois_dot_batch with g = 1, k = 1)                                                  -- the PARENT commit's library
  galois   k = 3, 8: `pair` = ntt_rns_galois_dot_pair_batch (this library) against `twice` = two ntt_rns_galois_dot_batch calls
           (the parent's library; `twice_cur`: the same two calls on this library), a rotation by 1, broadcast keys, accumulating
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, 24 limbs of 50-bit primes (runs of 16 and 8), digit (0, count), count in {1, 2, 3, 4, 8}, 2 / 64 / 1024
polynomials.  The two libraries run in ALTERNATING child processes on the same board, round by round; a child times every shape.
Inside a child the variants of a shape are timed INTERLEAVED, three windows each in an order that rotates from round to round, and a
variant's figure for the round is the median of its windows.  Printed per shape: the median ms per call of each variant; the parent's
own run-to-run spread over the rounds (max / min of the better baseline); and the call-rate ratios best(A, B) / variant as RANGES
over the rounds (round r of one library against round r of the other).  ntt_copy_probe of one operand (8 nl batch N bytes read, as
many written) in the same child for scale.  The one-call variants set NTT_OPT_PAIR_FUSED inside every timed call (one more host call
each).  Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
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
COUNTS = (0, 1, 4) if a.quick else (0, 1, 2, 3, 4, 8)  # 0: fwd_mul_pair
GALOIS_K = (3,) if a.quick else (3, 8)
BATCHES = (2, 64) if a.quick else (2, 64, 1024)
FLAGS = 2 | 4  # NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE
GFLAGS = 1 | 2 | 4  # NTT_GALOIS_TRANSFORMED | ACCUMULATE | KEY_BROADCAST


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"kind,count,batch,variant": ms per call} as one JSON line"""
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    plans = []
    for k in range(NL):
        q = lib.find_prime(50, n, k)
        plans.append(lib.Plan(n, q, lib.min_root(q, n)))
    top, kmax = max(BATCHES), max(GALOIS_K)
    dext, dc0, dc1 = (lib.DeviceBuffer(NL * top * n) for _ in range(3))
    dk = [lib.DeviceBuffer(NL * n) for _ in range(2 * kmax)]  # key0_i = dk[i], key1_i = dk[kmax + i]
    dig = [dext] + [lib.DeviceBuffer(NL * top * n) for _ in range(kmax - 1)]  # the Galois product's k digits
    for i, d in enumerate(dk):
        for l, p in enumerate(plans):
            lib.fill_uniform(d.ptr + 8 * l * n, n, p.q, 500 + 100 * i + l, 0)
    g = lib.galois_rotation(n, 1)
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

    def pair_call(opt, count, batch):
        def call():
            plans[0].set_option(lib.OPT_PAIR_FUSED, opt)
            if count:
                lib.rns_mod_up_mul_pair(plans, dc0.ptr, dc1.ptr, dext.ptr, 0, count, dk[0].ptr, dk[kmax].ptr, batch, FLAGS)
            else:
                lib.rns_fwd_mul_pair(plans, dc0.ptr, dc1.ptr, dext.ptr, dk[0].ptr, dk[kmax].ptr, batch, FLAGS)
        return call

    def twice(count, batch):
        def call():
            for c, key in ((dc0, dk[0]), (dc1, dk[kmax])):
                if count:
                    lib.rns_mod_up_mul(plans, c.ptr, dext.ptr, 0, count, key.ptr, batch, FLAGS)
                else:
                    lib.rns_fwd_mul(plans, c.ptr, dext.ptr, key.ptr, batch, FLAGS)
        return call

    def by_parts(count, batch):
        def call():
            if count:
                lib.rns_mod_up(plans, dext.ptr, 0, count, batch, 0)
            lib.rns_fwd(plans, dext.ptr, batch)
            for c, key in ((dc0, dk[0]), (dc1, dk[kmax])):
                lib.rns_galois_dot(plans, c.ptr, [dext.ptr], [key.ptr], 1, batch, GFLAGS)
        return call

    def dot_twice(k, batch):
        def call():
            for c, base in ((dc0, 0), (dc1, kmax)):
                lib.rns_galois_dot(plans, c.ptr, [d.ptr for d in dig[:k]], [d.ptr for d in dk[base:base + k]], g, batch, GFLAGS)
        return call

    def dot_pair(k, batch):
        def call():
            lib.rns_galois_dot_pair(plans, dc0.ptr, dc1.ptr, [d.ptr for d in dig[:k]], [d.ptr for d in dk[:k]],
                                    [d.ptr for d in dk[kmax:kmax + k]], g, batch, GFLAGS)
        return call

    out = {}
    for batch in BATCHES:
        per = batch * n
        for l, p in enumerate(plans):  # canonical words in every slot
            for i, d in enumerate(dig + [dc0, dc1]):
                lib.fill_uniform(d.ptr + 8 * l * per, per, p.q, 77 + 50 * i + l, 0)
        lib.stream_sync()
        out["copy,0,%d,copy" % batch] = interleaved({"copy": lambda: lib.copy_probe(dc0.ptr, dext.ptr, NL * per)})["copy"]
        for l, p in enumerate(plans):
            lib.fill_uniform(dc0.ptr + 8 * l * per, per, p.q, 177 + l, 0)
        for count in COUNTS:
            if which == "prev":
                fns = {"A": twice(count, batch), "B": by_parts(count, batch)}
            else:
                fns = {"fused": pair_call(1, count, batch), "comp": pair_call(0, count, batch), "auto": pair_call(-1, count, batch)}
            for name, ms in interleaved(fns).items():
                out["mul,%d,%d,%s" % (count, batch, name)] = ms
        for k in GALOIS_K:
            fns = {"twice": dot_twice(k, batch)} if which == "prev" else {"pair": dot_pair(k, batch), "twice_cur": dot_twice(k, batch)}
            for name, ms in interleaved(fns).items():
                out["galois,%d,%d,%s" % (k, batch, name)] = ms
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/key_pair_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# %d limbs of 50-bit primes, digit (0, count) (count 0: fwd_mul_pair, no conversion), broadcast keys, accumulating; %d rounds of" % (NL, ROUNDS))
    print("# alternating child processes, each timing the variants of a shape interleaved, %d windows each, in an order rotated by the round" % WINDOWS)
    print("# %d calls after %d warm-up calls per shape; ms = median over the rounds; best = min(A, B) per round of the PARENT's library;" % (CALLS, WARM))
    print("# ratios = best ms / variant ms, min..max over the rounds; spread = max / min of best over the rounds")
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
            cp = statistics.median([r["copy,0,%d,copy" % batch] for r in rounds["cur"]])
            print("copy     N=2^%d polys=%-5d ntt_copy_probe of one operand (%.1f MB read + written) %8.4f ms" % (
                logn, batch, 16.0 * NL * batch * (1 << logn) / 1e6, cp))
            for count in COUNTS:
                pa = [r["mul,%d,%d,A" % (count, batch)] for r in rounds["prev"]]
                pb = [r["mul,%d,%d,B" % (count, batch)] for r in rounds["prev"]]
                best = [min(x, y) for x, y in zip(pa, pb)]
                v = {name: [r["mul,%d,%d,%s" % (count, batch, name)] for r in rounds["cur"]] for name in ("fused", "comp", "auto")}
                ratio = {name: [p / t for p, t in zip(best, ts)] for name, ts in v.items()}
                print("key_pair N=2^%d polys=%-5d count=%d  parent A %8.4f ms  B %8.4f ms  best spread %.2f  fused %8.4f ms  comp %8.4f ms  "
                      "auto %8.4f ms  best/fused %s  best/comp %s  best/auto %s" % (
                          logn, batch, count, statistics.median(pa), statistics.median(pb), max(best) / min(best), statistics.median(v["fused"]),
                          statistics.median(v["comp"]), statistics.median(v["auto"]), rng(ratio["fused"]), rng(ratio["comp"]), rng(ratio["auto"])))
            for k in GALOIS_K:
                tw = [r["galois,%d,%d,twice" % (k, batch)] for r in rounds["prev"]]
                pr = [r["galois,%d,%d,pair" % (k, batch)] for r in rounds["cur"]]
                tc = [r["galois,%d,%d,twice_cur" % (k, batch)] for r in rounds["cur"]]
                print("galois   N=2^%d polys=%-5d k=%d      parent twice %8.4f ms (spread %.2f)  twice_cur %8.4f ms  pair %8.4f ms  twice/pair %s  "
                      "pair / copy %.2f" % (logn, batch, k, statistics.median(tw), max(tw) / min(tw), statistics.median(tc), statistics.median(pr),
                                           rng([p / t for p, t in zip(tw, pr)]), statistics.median(pr) / cp))
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
