#!/usr/bin/env python3
"""tools/lincomb_bench.py [--quick] [--prev LIB] [--logn 13 14]: the linear layer, ntt_rns_lincomb_batch, timed with device events after
warm-ups beside what a caller of the PARENT commit has:

  add      c = a + b: k = 2, everything else NULL                                                         -- this library
  comb4    c = 3 a0 + 5 a1 + 7 a2 + 11 a3 + bias: k = 4, per-limb scalars and bias                        -- this library
  copyadd, copycomb4   ntt_copy_probe moving the same algorithmic bytes (24 N and 40 N per limb-polynomial) -- this library
  add_t, comb4_t       the same two operations with torch integer ops on the same device buffers ((x + y), compare, subtract,
           select; the small scalars let torch's int64 hold the whole sum, so one remainder ends it: the cheapest form torch has --
           general scalars need a 128-bit product it lacks)                                                -- beside the PARENT's library
  gd3, gd8 sum_{i<k} pt_i (.) sigma_{g_i}(a), k = 3 and 8, broadcast multipliers, k DISTINCT g: one call   -- this library
           against k accumulating ntt_rns_galois_dot_batch calls (one pair each, KEY_BROADCAST)           -- the PARENT commit's library
  ge3, ge8 the same with all g EQUAL: one call                                                            -- this library
           against ONE ntt_rns_galois_dot_batch call with k pairs                                         -- the PARENT commit's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, 24 limbs of 50-bit primes, 2 / 64 / 1024 polynomials.  torch is imported first, so the library binds to the HIP
runtime torch loaded; every call and every torch op goes to ONE torch stream.  The two libraries run in ALTERNATING child processes on
the same board, round by round; a child times every shape.  Inside a child the variants of a shape are timed INTERLEAVED, three windows
each in an order that rotates from round to round, and a variant's figure for the round is the median of its windows.  Printed per
shape: the median ms per call of each variant; the parent's own run-to-run spread over the rounds (max / min of its figure); the
call-rate ratios parent / this library as RANGES over the rounds (round r of one library against round r of the other): a ratio inside
the spread counts as "not different"; and the copy probe's time over the call's (the call's rate as a fraction of the probe's)."""
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
NL = 24
BATCHES = (2, 64) if a.quick else (2, 64, 1024)
KS = (3, 8)
SCALARS, BIAS = (3, 5, 7, 11), 7
GT, GA, GB = 1, 2, 4  # NTT_GALOIS_TRANSFORMED, _ACCUMULATE, _KEY_BROADCAST
MB = 2                # NTT_LINCOMB_M_BROADCAST


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"batch,variant": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    qs = [lib.find_prime(50, n, k) for k in range(NL)]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    top = max(BATCHES)
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    pool = torch.empty(8 * NL * top * n, dtype=torch.int64, device="cuda:0")  # operands side by side: a0 a1 a2 a3 c, the probe's destination
    pts = torch.empty(max(KS) * NL * n, dtype=torch.int64, device="cuda:0")   # the broadcast multipliers, [limb][N] each
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gs = [pow(5, i + 1, 2 * n) for i in range(max(KS))]

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

    for i in range(max(KS)):
        for l in range(NL):
            lib.fill_uniform(pts.data_ptr() + 8 * (i * NL + l) * n, n, qs[l], 500 + 30 * i + l, 0, stream=sp)
    mp = [pts.data_ptr() + 8 * i * NL * n for i in range(max(KS))]
    out = {}
    for batch in BATCHES:
        per = batch * n
        op = NL * per  # words of one operand
        for o in range(5):
            for l in range(NL):
                lib.fill_uniform(pool.data_ptr() + 8 * (o * op + l * per), per, qs[l], 77 + 30 * o + l, 0, stream=sp)
        st.synchronize()
        p = [pool.data_ptr() + 8 * o * op for o in range(6)]  # p[5]: the probe's destination, 2.5 operands
        view = lambda o: pool[o * op:(o + 1) * op].view(NL, per)
        qcol = torch.tensor(qs, dtype=torch.int64, device="cuda:0").view(NL, 1)
        if which == "prev":
            def add_t():
                s = view(0) + view(1)
                torch.where(s >= qcol, s - qcol, s, out=view(4))

            def comb4_t():
                s = view(0) * SCALARS[0]
                for i in (1, 2, 3):
                    s.add_(view(i), alpha=SCALARS[i])
                s.add_(BIAS)
                torch.remainder(s, qcol, out=view(4))

            def dots(k):
                def f():
                    for i in range(k):
                        lib.rns_galois_dot(plans, p[4], [p[0]], [mp[i]], gs[i], batch, GT | GB | (GA if i else 0), stream=sp)
                return f

            def dot(k):
                return lambda: lib.rns_galois_dot(plans, p[4], [p[0]] * k, mp[:k], gs[0], batch, GT | GB, stream=sp)
            fns = {"add": add_t, "comb4": comb4_t}
            for k in KS:
                fns["gd%d" % k] = dots(k)
                fns["ge%d" % k] = dot(k)
        else:
            def lin(k, g):
                return lambda: lib.rns_lincomb(plans, p[4], [p[0]] * k, mp[:k], None, g, None, batch, MB, stream=sp)
            sc = [[s] * NL for s in SCALARS]
            fns = {"add": lambda: lib.rns_add(plans, p[4], p[0], p[1], batch, stream=sp),
                   "comb4": lambda: lib.rns_lincomb(plans, p[4], p[:4], None, sc, None, [BIAS] * NL, batch, 0, stream=sp),
                   # the same algorithmic bytes: 16 bytes per word copied -- 24 N per limb-polynomial is 1.5 operands, 40 N is 2.5
                   "copyadd": lambda: lib.copy_probe(p[5], p[0], op * 3 // 2, stream=sp),
                   "copycomb4": lambda: lib.copy_probe(p[5], p[0], op * 5 // 2, stream=sp)}
            for k in KS:
                fns["gd%d" % k] = lin(k, gs[:k])
                fns["ge%d" % k] = lin(k, [gs[0]] * k)
        for name, ms in interleaved(fns).items():
            out["%d,%s" % (batch, name)] = ms
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/lincomb_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# %d limbs of 50-bit primes; %d rounds of alternating child processes, each timing the variants of a shape interleaved," % (NL, ROUNDS))
    print("# %d windows each, in an order rotated by the round; %d calls after %d warm-up calls per window; ms = median over the rounds;" % (WINDOWS, CALLS, WARM))
    print("# parent/cur = parent ms / this library's ms, min..max over the rounds; spread = max / min of the parent's figure over the rounds;")
    print("# rate vs copy = the copy probe's ms (same algorithmic bytes) / the call's ms, min..max over the rounds")
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
        what = {"add": "add (k = 2) vs torch integer ops", "comb4": "4 scalar terms + bias vs torch integer ops",
                "gd3": "k = 3, distinct g vs 3 accumulating galois_dot calls", "gd8": "k = 8, distinct g vs 8 accumulating galois_dot calls",
                "ge3": "k = 3, equal g vs one galois_dot call", "ge8": "k = 8, equal g vs one galois_dot call"}
        for batch in BATCHES:
            for name in ("add", "comb4", "gd3", "gd8", "ge3", "ge8"):
                pv, cv = col("prev", "%d,%s" % (batch, name)), col("cur", "%d,%s" % (batch, name))
                line = "%-6s N=2^%d polys=%-5d parent %8.4f ms (spread %.2f)  lincomb %8.4f ms (spread %.2f)  parent/cur %s" % (
                    name, logn, batch, med(pv), max(pv) / min(pv), med(cv), max(cv) / min(cv), rng([x / y for x, y in zip(pv, cv)]))
                if name in ("add", "comb4"):
                    cp = col("cur", "%d,copy%s" % (batch, name))
                    line += "  copy probe %8.4f ms  rate vs copy %s" % (med(cp), rng([x / y for x, y in zip(cp, cv)]))
                print(line + "   # " + what[name])
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
