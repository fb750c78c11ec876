#!/usr/bin/env python3
"""tools/sample_bench.py [--quick] [--logn 13 14] [--out FILE]: the device-side sampler, ntt_rns_sample_batch, timed with device events
after warm-ups:

  (a) fused    NTT_SAMPLE_TRANSFORMED with NTT_OPT_SAMPLE_FUSED 1 (sample_fwd_kernel, one launch per run)
      comp     the same call with NTT_OPT_SAMPLE_FUSED 0 (sample_coef_kernel, then the forward transform; accumulating: the inverse
               transform first)
               for the two small kinds (ternary, cbd21), storing and accumulating
  (b) detour   what a caller of the parent commit has: the small values drawn with torch on the device (ternary: randint; cbd21: the
               difference of two binomial(21, 1/2) draws), reduced mod t, then ntt_rns_from_plain_batch with the same flags (its
               default route) -- against the fused kernel and against the composition
  (c) coef     the coefficient call (no NTT_SAMPLE_TRANSFORMED) per kind, storing
      copy     ntt_copy_probe moving the coefficient call's algorithmic bytes, 8 N L per polynomial

N = 2^13 and 2^14, L = 1, 4, 16 of 24 50-bit primes, 64 / 1024 polynomials.  torch is imported first, so the library binds to the HIP
runtime torch loaded; every call and every torch op goes to ONE torch stream.  Five rounds of fresh child processes, one per size and
round, the sizes alternating; a child times every shape.  Inside a child the variants of a shape are timed INTERLEAVED, three windows
each in an order that rotates from round to round, and a variant's figure for the round is the median of its windows.  Printed per
shape: the median ms per call of each variant, the spread of a figure over the rounds (max / min), and the ratios comp / fused,
detour / call and copy / call as RANGES over the rounds: a ratio inside the spread counts as "not different"."""
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
ap.add_argument("--logn", type=int, nargs="+", default=[13, 14])
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--child", nargs=2, metavar=("LOGN", "ROUND"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (5, 10, 3, 3)
LS = (1, 4) if a.quick else (1, 4, 16)
BATCHES = (64,) if a.quick else (64, 1024)
NPRIMES = 24
T = 65537
SEED = 0x5EED
TERNARY, CBD21, UNIFORM = 0, 1, 2
TRANSFORMED, ACCUMULATE = 2, 4
SMALL = (("ternary", TERNARY), ("cbd21", CBD21))


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(logn, rnd):
    """every shape once: {"batch,L,variant": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt
    lib = ontt.load()
    n = 1 << logn
    top_l, top_b = max(LS), max(BATCHES)
    qs = [lib.find_prime(50, n, k) for k in range(NPRIMES)]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs[:top_l]]
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    # the operand's limbs, then the detour's plaintext words, then the probe's destination
    pool = torch.empty(top_l * top_b * n + top_b * n + top_l * top_b * n // 2 + n, dtype=torch.int64, device="cuda:0")
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
    m_off = top_l * top_b * n
    dm, probe_dst = base + 8 * m_off, base + 8 * (m_off + top_b * n)
    for batch in BATCHES:
        per = batch * n
        m = pool[m_off:m_off + per]
        count21 = torch.full((per,), 21.0, device="cuda:0")
        half = torch.full((per,), 0.5, device="cuda:0")
        for nl in LS:
            for l in range(nl):
                lib.fill_uniform(base + 8 * l * per, per, qs[l], 77 + l, 0, stream=sp)
            st.synchronize()
            ps = plans[:nl]

            def call(kind, flags, fused):
                def run():
                    ps[0].set_option(lib.OPT_SAMPLE_FUSED, fused)
                    lib.rns_sample(ps, base, kind, SEED, batch, flags=flags, stream=sp)
                return run

            def detour(kind, flags):
                def run():
                    if kind == TERNARY:
                        v = torch.randint(-1, 2, (per,), device="cuda:0", dtype=torch.int64)
                    else:
                        v = (torch.binomial(count21, half) - torch.binomial(count21, half)).to(torch.int64)
                    torch.remainder(v, T, out=m)
                    lib.rns_from_plain(ps, base, dm, T, batch, flags, stream=sp)
                return run

            fns = {}
            for name, kind in SMALL:
                for acc, tag in ((0, "store"), (ACCUMULATE, "acc")):
                    fns["%s/%s/fused" % (name, tag)] = call(kind, TRANSFORMED | acc, 1)
                    fns["%s/%s/comp" % (name, tag)] = call(kind, TRANSFORMED | acc, 0)
                    fns["%s/%s/detour" % (name, tag)] = detour(kind, TRANSFORMED | acc)
            for name, kind in SMALL + (("uniform", UNIFORM),):
                fns["%s/coef" % name] = call(kind, 0, -1)
            # 16 bytes per word copied: 8 N L per polynomial is L / 2 polynomials
            fns["copy"] = lambda: lib.copy_probe(probe_dst, base, max(per * nl // 2, 1), stream=sp)
            for name, ms in interleaved(fns).items():
                out["%d,%d,%s" % (batch, nl, name)] = ms
            ps[0].set_option(lib.OPT_SAMPLE_FUSED, -1)
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    lines = []

    def say(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)

    say("# tools/sample_bench.py  library sha256 %s" % sha(cur))
    say("# the first L of %d 50-bit primes, seed 0x%X, detour with t = %d; %d rounds of fresh child processes (the sizes alternating)," % (NPRIMES, SEED, T, ROUNDS))
    say("# each timing the variants of a shape interleaved, %d windows each, in an order rotated by the round; %d calls after %d warm-up" % (WINDOWS, CALLS, WARM))
    say("# calls per window; ms = median over the rounds; comp/fused = the composition's ms / the fused kernel's ms, min..max over the")
    say("# rounds (above 1: the fused kernel is faster); detour/x likewise; spread = max / min of a figure over the rounds;")
    say("# rate vs copy = the copy probe's ms at the call's algorithmic bytes (8 N L per polynomial) / the call's ms")
    rounds = {logn: [] for logn in a.logn}
    for rnd in range(ROUNDS):
        for logn in a.logn:
            args = [sys.executable, os.path.abspath(__file__), "--child", str(logn), str(rnd)] + (["--quick"] if a.quick else [])
            r = subprocess.run(["timeout", "-k", "10", "300"] + args, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("child 2^%d round %d failed (%d): %s" % (logn, rnd, r.returncode, r.stderr[-2000:]))
            rounds[logn].append(json.loads(r.stdout.strip().splitlines()[-1]))
    med = statistics.median
    for logn in a.logn:
        col = lambda key: [r[key] for r in rounds[logn]]
        for batch in BATCHES:
            for nl in LS:
                key = "%d,%d," % (batch, nl)
                head = "N=2^%d polys=%-5d L=%-2d " % (logn, batch, nl)
                cp = col(key + "copy")
                for name, _ in SMALL:
                    for tag in ("store", "acc"):
                        fu, co, de = (col(key + "%s/%s/%s" % (name, tag, v)) for v in ("fused", "comp", "detour"))
                        say("(a) %s %-7s %-5s fused %8.4f ms (spread %.2f)  comp %8.4f ms (spread %.2f)  comp/fused %s  rate vs copy %s" % (
                            head, name, tag, med(fu), max(fu) / min(fu), med(co), max(co) / min(co), rng([x / y for x, y in zip(co, fu)]),
                            rng([x * (2 if tag == "acc" else 1) / y for x, y in zip(cp, fu)])))
                        say("(b) %s %-7s %-5s detour %8.4f ms (spread %.2f)  detour/fused %s  detour/comp %s" % (
                            head, name, tag, med(de), max(de) / min(de), rng([x / y for x, y in zip(de, fu)]), rng([x / y for x, y in zip(de, co)])))
                for name in ("ternary", "cbd21", "uniform"):
                    cf = col(key + "%s/coef" % name)
                    say("(c) %s %-7s coef  store %8.4f ms (spread %.2f)  copy probe %8.4f ms  rate vs copy %s" % (
                        head, name, med(cf), max(cf) / min(cf), med(cp), rng([x / y for x, y in zip(cp, cf)])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.child:
    child(int(a.child[0]), int(a.child[1]))
else:
    main()
