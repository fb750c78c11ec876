#!/usr/bin/env python3
"""tools/slots_bench.py [--quick] [--prev LIB] [--logn 13 14]: BFV / BGV slot encode and decode, ntt_slots_encode_batch and
ntt_slots_decode_batch, timed with device events after warm-ups:

  fused    NTT_OPT_SLOTS_FUSED 1 (slots_inv_kernel / slots_fwd_kernel, one launch)                                 -- this library
  comp     NTT_OPT_SLOTS_FUSED 0 (slots_perm_kernel and the plan's transform in place)                             -- this library
  copy     ntt_copy_probe moving the call's algorithmic bytes, 16 N per polynomial                                 -- this library
  detour   what a caller of the PARENT commit has: a torch gather (index_select with a precomputed index tensor, derived on the
           host) and ntt_inv_batch / ntt_fwd_batch                                                                 -- the PARENT's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

t = 65537, N = 2^13 and 2^14, 64 / 1024 polynomials.  torch is imported first, so the library binds to the HIP runtime torch loaded;
every call and every torch op goes to ONE torch stream.  The two libraries run in ALTERNATING child processes on the same board,
round by round; a child times every shape.  Inside a child the variants of a shape are timed INTERLEAVED, three windows each in an
order that rotates from round to round, and a variant's figure for the round is the median of its windows.  Printed per shape and
direction: the median ms per call of each variant, the spread of a figure over the rounds (max / min), and the ratios comp / fused,
copy / call and detour / fused as RANGES over the rounds: a ratio inside the spread counts as "not different"."""
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
ap.add_argument("--no-prev", action="store_true", help="skip the detour")
ap.add_argument("--logn", type=int, nargs="+", default=[13, 14])
ap.add_argument("--child", nargs=3, metavar=("WHICH", "LOGN", "ROUND"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (5, 10, 3, 3)
BATCHES = (64,) if a.quick else (64, 1024)
T = 65537
OPT_SLOTS_FUSED = 23
DIRS = ("encode", "decode")


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def pos_table(n):
    """pos(i) = bitrev_m((e(i) - 1) / 2), e(i) = +-5^j mod 2N: what the parent's caller has to derive on its own"""
    m, h = n.bit_length() - 1, n // 2
    row0 = [pow(5, j, 2 * n) for j in range(h)]
    return [int(format((e - 1) // 2, "0%db" % m)[::-1], 2) for e in row0 + [2 * n - e for e in row0]]


def child(which, logn, rnd):
    """every shape once: {"batch,direction,variant": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n, top_b = 1 << logn, max(BATCHES)
    plan = lib.Plan(n, T, lib.min_root(T, n))
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    pool = torch.empty(2 * top_b * n, dtype=torch.int64, device="cuda:0")  # the slot side, then the coefficient side
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if which == "prev":
        pos = torch.tensor(pos_table(n), dtype=torch.int64, device="cuda:0")
        ipos = torch.empty_like(pos)
        ipos[pos] = torch.arange(n, dtype=torch.int64, device="cuda:0")
    else:
        plan.enable_slots()

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
    dv = pool.data_ptr()
    for batch in BATCHES:
        per = batch * n
        da = dv + 8 * top_b * n
        # canonical words on both sides; every call below maps canonical words to canonical words, so they stay valid inputs
        lib.fill_uniform(dv, per, T, 5, 0, stream=sp)
        lib.fill_uniform(da, per, T, 6, 0, stream=sp)
        st.synchronize()
        if which == "prev":
            v2, a2 = pool[:per].view(batch, n), pool[top_b * n:top_b * n + per].view(batch, n)

            def enc_detour():
                with torch.cuda.stream(st):
                    torch.index_select(v2, 1, ipos, out=a2)
                plan.inv(da, batch, stream=sp)

            def dec_detour():
                plan.fwd(da, batch, stream=sp)
                with torch.cuda.stream(st):
                    torch.index_select(a2, 1, pos, out=v2)
            fns = {"encode/detour": enc_detour, "decode/detour": dec_detour}
        else:
            def call(direction, fused):
                def run():
                    plan.set_option(OPT_SLOTS_FUSED, fused)
                    if direction == "encode":
                        lib.slots_encode(plan, da, dv, batch, stream=sp)
                    else:
                        lib.slots_decode(plan, dv, da, batch, stream=sp)
                return run
            fns = {"%s/%s" % (d, tag): call(d, f) for d in DIRS for tag, f in (("fused", 1), ("comp", 0))}
            fns["copy"] = lambda: lib.copy_probe(da, dv, per, stream=sp)  # 16 bytes per word copied: 16 N per polynomial
        for name, ms in interleaved(fns).items():
            out["%d,%s" % (batch, name)] = ms
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    prev = not a.no_prev and os.path.exists(a.prev)
    print("# tools/slots_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s" % ("%s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)) if prev else "not measured (the detour skipped)"))
    print("# t = %d; %d rounds of alternating child processes, each timing the variants of a shape interleaved, %d windows each, in an order" % (T, ROUNDS, WINDOWS))
    print("# rotated by the round; %d calls after %d warm-up calls per window; ms = median over the rounds; comp/fused = the composition's ms /" % (CALLS, WARM))
    print("# the fused kernel's ms, min..max over the rounds (above 1: the fused kernel is faster); spread = max / min of a figure over the")
    print("# rounds; rate vs copy = the copy probe's ms (16 N bytes per polynomial) / the call's ms")
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
                r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("child %s 2^%d failed (%d): %s" % (which, logn, r.returncode, r.stderr[-2000:]))
                rounds[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
        col = lambda which, key: [r[key] for r in rounds[which]]
        med = statistics.median
        for batch in BATCHES:
            cp = col("cur", "%d,copy" % batch)
            for d in DIRS:
                fu, co = col("cur", "%d,%s/fused" % (batch, d)), col("cur", "%d,%s/comp" % (batch, d))
                line = "N=2^%d polys=%-5d %-6s fused %8.4f ms (spread %.2f)  comp %8.4f ms (spread %.2f)  comp/fused %s  copy probe %8.4f ms  rate vs copy: fused %s comp %s" % (
                    logn, batch, d, med(fu), max(fu) / min(fu), med(co), max(co) / min(co), rng([x / y for x, y in zip(co, fu)]), med(cp),
                    rng([x / y for x, y in zip(cp, fu)]), rng([x / y for x, y in zip(cp, co)]))
                if prev:
                    pv = col("prev", "%d,%s/detour" % (batch, d))
                    line += "  parent's detour %8.4f ms (spread %.2f)  detour/fused %s  detour/comp %s" % (
                        med(pv), max(pv) / min(pv), rng([x / y for x, y in zip(pv, fu)]), rng([x / y for x, y in zip(pv, co)]))
                print(line)
        sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
