#!/usr/bin/env python3
"""tools/exact_bench.py [--quick] [--prev LIB] [--logn 13 14]: the exact base conversions of BFV multiplication, timed with device events
after warm-ups:

  (a) up      ntt_rns_mod_up_exact_batch, coefficients, 24 limbs of 50-bit primes, digit (0, count), count 1 / 4 / 8   -- this library
      up0     ntt_rns_mod_up_batch at the same shape: the price of the correction                             -- the PARENT commit's library
  (b) fused   ntt_rns_mod_down_exact_batch, TRANSFORMED, mult 65537, NTT_OPT_RESCALE_FUSED 1, np 1 / 2 / 4 / 8        -- this library
              (the library's rule takes the fused kernel up to np 4: the np 8 row of this column reads the sandwich unless
              kExactFusedMaxNp in host/host_exact.inc is raised for the measurement, as it was for profiles/r15/exact_bench.txt)
      sand    the same call, NTT_OPT_RESCALE_FUSED 0 (inverse, coefficient kernel, forward)
      down0   ntt_rns_mod_down_batch, TRANSFORMED, at the same shape                                           -- the PARENT commit's library
  (c) bfv     the five calls of examples/rns_bfv_mul.c (R = 5, Q = 4 limbs of 50-bit primes, t = 65537)               -- this library
      bfv0    the same sequence from the approximate calls: ntt_rns_mod_up_batch, ntt_rns_tensor_batch, the R limbs times t with
              torch integer ops (t = 2^16 + 1: two shifts by 8 with a remainder each, one add, one select), ntt_rns_mod_down_batch,
              ntt_rns_mod_up_batch                                                                             -- the PARENT commit's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

N = 2^13 and 2^14, 2 / 64 / 1024 polynomials ((c): polynomials / 4 multiplications, at least one; a multiplication has 4 input and 3
output polynomials).  torch is imported first, so the library binds to the HIP runtime torch
loaded; every call and every torch op goes to ONE torch stream.  The two libraries run in ALTERNATING child processes on the same board,
round by round; inside a child the variants of a shape are timed INTERLEAVED, three windows each in an order that rotates from round to
round, and a variant's figure for the round is the median of its windows.  Printed per shape: the median ms per call of each variant, the
parent's own run-to-run spread over the rounds (max / min of its figure) and the call-rate ratios as RANGES over the rounds."""
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
COUNTS = (4,) if a.quick else (1, 4, 8)
NPS = (2,) if a.quick else (1, 2, 4, 8)
BATCHES = (2, 64) if a.quick else (2, 64, 1024)
NR, NQ, TMOD = 5, 4, 65537
T = 1


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"kind,parameter,batch,variant": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    qs = [lib.find_prime(50, n, k) for k in range(NL)] + [lib.find_prime(60, n, k) for k in range(max(NPS))]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    top = max(BATCHES)
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    buf = torch.empty((NL + max(NPS)) * top * n, dtype=torch.int64, device="cuda:0")
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
        for l, q in enumerate(qs):  # canonical words in every slot (they stay canonical under every call timed here)
            lib.fill_uniform(buf.data_ptr() + 8 * l * per, per, q, 77 + l, 0, stream=sp)
        st.synchronize()
        for count in COUNTS:
            if which == "prev":
                fns = {"up0": lambda: lib.rns_mod_up(plans[:NL], buf.data_ptr(), 0, count, batch, 0, stream=sp)}
            else:
                fns = {"up": lambda: lib.rns_mod_up_exact(plans[:NL], buf.data_ptr(), 0, count, batch, 0, stream=sp)}
            for name, ms in interleaved(fns).items():
                out["up,%d,%d,%s" % (count, batch, name)] = ms
        for np_ in NPS:
            ps = plans[:NL] + plans[NL:NL + np_]
            if which == "prev":
                fns = {"down0": lambda: lib.rns_mod_down(ps, np_, buf.data_ptr(), batch, T, stream=sp)}
            else:
                def call(opt):
                    def f():
                        plans[0].set_option(lib.OPT_RESCALE_FUSED, opt)
                        lib.rns_mod_down_exact(ps, np_, buf.data_ptr(), TMOD, batch, T, stream=sp)
                    return f
                fns = {"fused": call(1), "sand": call(0)}
            for name, ms in interleaved(fns).items():
                out["down,%d,%d,%s" % (np_, batch, name)] = ms
        plans[0].set_option(lib.OPT_RESCALE_FUSED, -1)
        # (c) batch / 4 multiplications, 4 input and 3 output polynomials of [9][N] each
        muls = max(1, batch // 4)
        bp, poly = plans[:NR + NQ], (NR + NQ) * n
        din = torch.empty(4 * muls * poly, dtype=torch.int64, device="cuda:0")
        dd = torch.empty(3 * muls * poly, dtype=torch.int64, device="cuda:0")
        for j in range(4 * muls):
            for l in range(NR + NQ):
                lib.fill_uniform(din.data_ptr() + 8 * (j * poly + l * n), n, qs[l], 300 + l, 0, stream=sp)
        st.synchronize()
        lay = (n, poly)
        # operand-major: [4][muls][9][N] and [3][muls][9][N], so ONE tensor call serves every multiplication
        o = [dd.data_ptr() + 8 * j * muls * poly for j in range(3)]
        i = [din.data_ptr() + 8 * j * muls * poly for j in range(4)]
        rq = torch.tensor(qs[:NR], dtype=torch.int64, device="cuda:0").view(1, NR, 1)
        dview = dd.view(3 * muls, NR + NQ, n)[:, :NR, :]

        def tensor():
            lib.rns_tensor(bp, o[0], o[1], o[2], i[0], i[1], i[2], i[3], muls, 0, stream=sp, layout=lay)

        def times_t():
            x = dview
            y = torch.remainder(torch.remainder(x << 8, rq) << 8, rq) + x
            dview.copy_(torch.where(y >= rq, y - rq, y))

        def bfv():
            lib.rns_mod_up_exact(bp, din.data_ptr(), NR, NQ, 4 * muls, T, stream=sp, layout=lay)
            tensor()
            lib.rns_mod_down_exact(bp, NQ, dd.data_ptr(), TMOD, 3 * muls, T, stream=sp, layout=lay)
            lib.rns_mod_up_exact(bp, dd.data_ptr(), 0, NR, 3 * muls, T, stream=sp, layout=lay)

        def bfv0():
            lib.rns_mod_up(bp, din.data_ptr(), NR, NQ, 4 * muls, T, stream=sp, layout=lay)
            tensor()
            times_t()
            lib.rns_mod_down(bp, NQ, dd.data_ptr(), 3 * muls, T, stream=sp, layout=lay)
            lib.rns_mod_up(bp, dd.data_ptr(), 0, NR, 3 * muls, T, stream=sp, layout=lay)

        name, fn = ("bfv0", bfv0) if which == "prev" else ("bfv", bfv)
        out["bfv,%d,%d,%s" % (muls, batch, name)] = interleaved({name: fn})[name]
        del din, dd
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/exact_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# (a), (b): %d limbs of 50-bit primes, np 60-bit P primes; (c): R = %d, Q = %d limbs of 50-bit primes, t = %d; %d rounds of alternating" % (NL, NR, NQ, TMOD, ROUNDS))
    print("# child processes, each timing the variants of a shape interleaved, %d windows each, in an order rotated by the round; %d calls after" % (WINDOWS, CALLS))
    print("# %d warm-up calls per window; ms = median over the rounds; ratios = call rates, min..max over the rounds; spread = max / min of the" % WARM)
    print("# parent's figure")
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
            for count in COUNTS:
                k = "up,%d,%d," % (count, batch)
                p, c = col("prev", k + "up0"), col("cur", k + "up")
                print("(a) up   N=2^%d polys=%-5d count=%d  parent ModUp %8.4f ms (spread %.2f)  exact %8.4f ms  parent/exact %s" % (
                    logn, batch, count, med(p), max(p) / min(p), med(c), rng([x / y for x, y in zip(p, c)])))
            for np_ in NPS:
                k = "down,%d,%d," % (np_, batch)
                p, f, s = col("prev", k + "down0"), col("cur", k + "fused"), col("cur", k + "sand")
                print("(b) down N=2^%d polys=%-5d np=%d     parent ModDown %8.4f ms (spread %.2f)  fused %8.4f ms  sandwich %8.4f ms  sandwich/fused %s  "
                      "parent/fused %s  parent/sandwich %s" % (logn, batch, np_, med(p), max(p) / min(p), med(f), med(s),
                                                               rng([x / y for x, y in zip(s, f)]), rng([x / y for x, y in zip(p, f)]),
                                                               rng([x / y for x, y in zip(p, s)])))
            muls = max(1, batch // 4)
            k = "bfv,%d,%d," % (muls, batch)
            p, c = col("prev", k + "bfv0"), col("cur", k + "bfv")
            print("(c) bfv  N=2^%d polys=%-5d muls=%-4d parent's approximate sequence %8.4f ms (spread %.2f)  exact sequence %8.4f ms  parent/exact %s" % (
                logn, batch, muls, med(p), max(p) / min(p), med(c), rng([x / y for x, y in zip(p, c)])))
            sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
