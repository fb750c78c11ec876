#!/usr/bin/env python3
"""tools/lift_bench.py [--quick] [--prev LIB] [--logn 13 14]: the lifts into the RNS, ntt_rns_from_plain_batch and
ntt_rns_from_double_batch, timed with device events after warm-ups:

  (a) fused    NTT_LIFT_TRANSFORMED with NTT_OPT_LIFT_FUSED 1 (lift_fwd_kernel, one launch per run)            -- this library
      comp     the same call with NTT_OPT_LIFT_FUSED 0 (lift_coef_kernel, then the forward transform; accumulating: the inverse
               transform first)                                                                              -- this library
               for the three modes (centred, scaled, double), storing and accumulating
  (b) coef     the coefficient call (no NTT_LIFT_TRANSFORMED), centred, storing                              -- this library
      copy_c   ntt_copy_probe moving the coefficient call's algorithmic bytes, 8 N (L + 1) per polynomial
      copy_f   ntt_copy_probe moving the fused call's algorithmic bytes, 8 N (L + 1) as well (storing)
  (c) detour   what a caller of the PARENT commit has for the centred NTT-domain lift: the spread with torch integer ops (compare,
               subtract, select, one remainder per limb into the operand) and ntt_rns_fwd_batch               -- the PARENT commit's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, L = 1, 4, 16 limbs of 50-bit primes, t = 65537, 64 / 1024 polynomials.  torch is imported first, so the library
binds to the HIP runtime torch loaded; every call and every torch op goes to ONE torch stream.  The two libraries run in ALTERNATING
child processes on the same board, round by round; a child times every shape.  Inside a child the variants of a shape are timed
INTERLEAVED, three windows each in an order that rotates from round to round, and a variant's figure for the round is the median of
its windows.  Printed per shape: the median ms per call of each variant, the spread of a figure over the rounds (max / min), and the
ratios comp / fused, copy / call and detour / fused as RANGES over the rounds: a ratio inside the spread counts as "not different"."""
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
ap.add_argument("--no-prev", action="store_true", help="skip variant (c)")
ap.add_argument("--logn", type=int, nargs="+", default=[13, 14])
ap.add_argument("--child", nargs=3, metavar=("WHICH", "LOGN", "ROUND"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (5, 10, 3, 3)
LS = (1, 4) if a.quick else (1, 4, 16)
BATCHES = (64,) if a.quick else (64, 1024)
T = 65537
SCALE, TRANSFORMED, ACCUMULATE = 1, 2, 4
MODES = (("centred", 0), ("scaled", SCALE), ("double", 0))


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
    qs = [lib.find_prime(50, n, k) for k in range(top_l)]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    # the operand's limbs, then the plaintext words, the doubles, the probe's destination
    pool = torch.empty(top_l * top_b * n + 2 * top_b * n + (top_l + 1) * top_b * n // 2 + n, dtype=torch.int64, device="cuda:0")
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
    base = pool.data_ptr()
    for batch in BATCHES:
        per = batch * n
        m_off, y_off = top_l * top_b * n, top_l * top_b * n + top_b * n
        dm, dy, probe_dst = base + 8 * m_off, base + 8 * y_off, base + 8 * (y_off + top_b * n)
        lib.fill_uniform(dm, per, T, 5, 0, stream=sp)
        with torch.cuda.stream(st):
            pool[y_off:y_off + per].view(torch.float64).copy_((pool[m_off:m_off + per] - T // 2).to(torch.float64) / 64.0)
        for nl in LS:
            for l in range(nl):
                lib.fill_uniform(base + 8 * l * per, per, qs[l], 77 + l, 0, stream=sp)
            st.synchronize()
            ps = plans[:nl]
            if which == "prev":
                m, half = pool[m_off:m_off + per], (T + 1) // 2
                dst = [pool[l * per:(l + 1) * per] for l in range(nl)]

                def detour():
                    mc = torch.where(m >= half, m - T, m)
                    for l in range(nl):
                        torch.remainder(mc, qs[l], out=dst[l])
                    lib.rns_fwd(ps, base, batch, stream=sp)
                fns = {"detour": detour}
            else:
                def call(kind, flags, fused):
                    def run():
                        ps[0].set_option(lib.OPT_LIFT_FUSED, fused)
                        if kind == "double":
                            lib.rns_from_double(ps, base, dy, 2.0 ** 30, batch, flags, stream=sp)
                        else:
                            lib.rns_from_plain(ps, base, dm, T, batch, flags, stream=sp)
                    return run
                fns = {}
                for kind, fl in MODES:
                    for acc, tag in ((0, "store"), (ACCUMULATE, "acc")):
                        fns["%s/%s/fused" % (kind, tag)] = call(kind, fl | TRANSFORMED | acc, 1)
                        fns["%s/%s/comp" % (kind, tag)] = call(kind, fl | TRANSFORMED | acc, 0)
                fns["coef"] = call("centred", 0, -1)
                # 16 bytes per word copied: 8 N (L + 1) per polynomial is (L + 1) / 2 polynomials
                fns["copy"] = lambda: lib.copy_probe(probe_dst, base, per * (nl + 1) // 2, stream=sp)
            for name, ms in interleaved(fns).items():
                out["%d,%d,%s" % (batch, nl, name)] = ms
            if which != "prev":
                ps[0].set_option(lib.OPT_LIFT_FUSED, -1)
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    prev = not a.no_prev and os.path.exists(a.prev)
    print("# tools/lift_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s" % ("%s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)) if prev else "not measured (variant (c) skipped)"))
    print("# 50-bit primes, t = %d, Delta = 2^30; %d rounds of alternating child processes, each timing the variants of a shape interleaved," % (T, ROUNDS))
    print("# %d windows each, in an order rotated by the round; %d calls after %d warm-up calls per window; ms = median over the rounds;" % (WINDOWS, CALLS, WARM))
    print("# comp/fused = the composition's ms / the fused kernel's ms, min..max over the rounds (above 1: the fused kernel is faster);")
    print("# spread = max / min of a figure over the rounds; rate vs copy = the copy probe's ms (8 N (L + 1) bytes per polynomial) / the call's ms")
    for logn in a.logn:
        rounds = {"prev": [], "cur": []}
        for rnd in range(ROUNDS):
            for which in (("prev", "cur") if prev else ("cur",)):
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
                head = "N=2^%d polys=%-5d L=%-2d " % (logn, batch, nl)
                cp = col("cur", key + "copy")
                for kind, _ in MODES:
                    for tag in ("store", "acc"):
                        fu, co = col("cur", key + "%s/%s/fused" % (kind, tag)), col("cur", key + "%s/%s/comp" % (kind, tag))
                        line = "(a) %s %-7s %-5s fused %8.4f ms (spread %.2f)  comp %8.4f ms (spread %.2f)  comp/fused %s" % (
                            head, kind, tag, med(fu), max(fu) / min(fu), med(co), max(co) / min(co), rng([x / y for x, y in zip(co, fu)]))
                        if kind == "centred" and tag == "store":
                            line += "  rate vs copy %s" % rng([x / y for x, y in zip(cp, fu)])
                            if prev:
                                pv = col("prev", key + "detour")
                                line += "  (c) parent's detour %8.4f ms (spread %.2f)  detour/fused %s" % (med(pv), max(pv) / min(pv), rng([x / y for x, y in zip(pv, fu)]))
                        print(line)
                cf = col("cur", key + "coef")
                print("(b) %s coef    store       %8.4f ms (spread %.2f)  copy probe %8.4f ms  rate vs copy %s" % (
                    head, med(cf), max(cf) / min(cf), med(cp), rng([x / y for x, y in zip(cp, cf)])))
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
