#!/usr/bin/env python3
"""tools/plain_bench.py [--quick] [--prev LIB] [--logn 13 14]: the conversions out of the RNS, ntt_rns_to_plain_batch, timed with device
events after warm-ups beside what a caller of the PARENT commit has:

  centred  m = [x_c]_t: flags 0                                                                         -- this library
  scale    m = round(t x / Q) mod t: NTT_PLAIN_SCALE                                                    -- this library
  copy     ntt_copy_probe moving the same algorithmic bytes, 8 N (L + 1) per polynomial                 -- this library
  detour   the SCALE result as the parent commit can express it, through an auxiliary 50-bit NTT prime r > t held as limb 0 of an
           [r, q_0 .. q_{L-1}] operand: ntt_rns_mod_up_exact_batch Q -> r, ntt_rns_mod_down_exact_batch with Q divided out and mult = t
           onto r, then the centred reduction mod t with torch integer ops (compare, subtract, select, remainder)
                                                                                                         -- the PARENT commit's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, L = 1, 4, 16 limbs of 50-bit primes, t = 65537, 64 / 1024 polynomials, coefficients.  torch is imported first, so
the library binds to the HIP runtime torch loaded; every call and every torch op goes to ONE torch stream.  The two libraries run in
ALTERNATING child processes on the same board, round by round; a child times every shape.  Inside a child the variants of a shape are
timed INTERLEAVED, three windows each in an order that rotates from round to round, and a variant's figure for the round is the median
of its windows.  Printed per shape: the median ms per call of each variant; the parent's own run-to-run spread over the rounds
(max / min of its figure); the call-rate ratio parent / this library as a RANGE over the rounds (round r of one library against round r
of the other): a ratio inside the spread counts as "not different"; and the copy probe's time over the call's (the call's rate as a
fraction of the probe's)."""
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
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (5, 10, 3, 3)
LS = (1, 4) if a.quick else (1, 4, 16)
BATCHES = (64,) if a.quick else (64, 1024)
T = 65537
SCALE = 1  # NTT_PLAIN_SCALE


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"batch,L,variant": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    top_l, top_b = max(LS), max(BATCHES)
    qs = [lib.find_prime(50, n, k) for k in range(top_l + 1)]  # the last one is the detour's r
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    r = qs[top_l]
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    # limb 0: the detour's r limb (this library: the output); limbs 1 .. L: the operand; then the probe's destination
    pool = torch.empty((top_l + 1) * top_b * n + (top_l + 1) * top_b * n // 2 + n, dtype=torch.int64, device="cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        with torch.cuda.stream(st):
            e0.record(st)
            for _ in range(CALLS):
                fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS

    def interleaved(fns):
        names = sorted(fns)
        names = names[rnd % len(names):] + names[:rnd % len(names)]
        with torch.cuda.stream(st):
            for name in names:
                for _ in range(WARM):
                    fns[name]()
        st.synchronize()
        t = {name: [] for name in names}
        for _ in range(WINDOWS):
            for name in names:
                t[name].append(window(fns[name]))
        return {name: statistics.median(v) for name, v in t.items()}

    out = {}
    for batch in BATCHES:
        per = batch * n
        for nl in LS:
            for l in range(nl):
                lib.fill_uniform(pool.data_ptr() + 8 * (l + 1) * per, per, qs[l], 77 + l, 0, stream=sp)
            st.synchronize()
            base = pool.data_ptr()
            if which == "prev":
                dplans = [plans[top_l]] + plans[:nl]
                y, half = pool[:per], r // 2

                def detour():
                    lib.rns_mod_up_exact(dplans, base, 1, nl, batch, 0, stream=sp)
                    lib.rns_mod_down_exact(dplans, nl, base, T, batch, 0, stream=sp)
                    torch.remainder(torch.where(y > half, y - r, y), T, out=y)
                fns = {"scale": detour}
            else:
                src, probe_dst = base + 8 * per, base + 8 * (top_l + 1) * top_b * n
                fns = {"centred": lambda: lib.rns_to_plain(plans[:nl], base, src, T, batch, 0, stream=sp),
                       "scale": lambda: lib.rns_to_plain(plans[:nl], base, src, T, batch, SCALE, stream=sp),
                       # the same algorithmic bytes: 16 bytes per word copied -- 8 N (L + 1) per polynomial is (L + 1) / 2 polynomials
                       "copy": lambda: lib.copy_probe(probe_dst, src, per * (nl + 1) // 2, stream=sp)}
            for name, ms in interleaved(fns).items():
                out["%d,%d,%s" % (batch, nl, name)] = ms
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/plain_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# 50-bit primes, t = %d; %d rounds of alternating child processes, each timing the variants of a shape interleaved," % (T, ROUNDS))
    print("# %d windows each, in an order rotated by the round; %d calls after %d warm-up calls per window; ms = median over the rounds;" % (WINDOWS, CALLS, WARM))
    print("# detour/scale = the parent's detour ms / this library's SCALE ms, min..max over the rounds; spread = max / min of a figure over the rounds;")
    print("# rate vs copy = the copy probe's ms (same algorithmic bytes, 8 N (L + 1) per polynomial) / the call's ms, min..max over the rounds")
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
        col = lambda which, key: [r[key] for r in rounds[which]]
        med = statistics.median
        for batch in BATCHES:
            for nl in LS:
                key = "%d,%d," % (batch, nl)
                pv, cp = col("prev", key + "scale"), col("cur", key + "copy")
                for mode in ("centred", "scale"):
                    cv = col("cur", key + mode)
                    line = "%-7s N=2^%d polys=%-5d L=%-2d  to_plain %8.4f ms (spread %.2f)  copy probe %8.4f ms  rate vs copy %s" % (
                        mode, logn, batch, nl, med(cv), max(cv) / min(cv), med(cp), rng([x / y for x, y in zip(cp, cv)]))
                    if mode == "scale":
                        line += "  parent's detour %8.4f ms (spread %.2f)  detour/scale %s" % (med(pv), max(pv) / min(pv), rng([x / y for x, y in zip(pv, cv)]))
                    print(line)
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
