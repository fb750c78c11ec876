#!/usr/bin/env python3
"""tools/bgv_bench.py [--quick] [--prev LIB] [--logn 13 14]: the BGV ModDown (ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch),
timed with device events after warm-ups, on the protocol of tools/exact_bench.py:

  down   fused   ntt_rns_mod_down_bgv_batch, TRANSFORMED, T = 65537, NTT_OPT_BGV_FUSED 1 (the fused kernel at any np)      -- this library
         sand    the same call, NTT_OPT_BGV_FUSED 0 (inverse, moddown_coef_kernel with the BGV constants, forward)
         down0   ntt_rns_mod_down_batch, TRANSFORMED, at the same shape: the price of the correction             -- the PARENT commit's library
  add    fused   ntt_rns_mod_down_bgv_add_batch, TRANSFORMED | ACCUMULATE, NTT_OPT_BGV_FUSED 1                            -- this library
         sand    the same call, NTT_OPT_BGV_FUSED 0 (the sandwich in place on the accumulator, then ct_fold_kernel)
         add0    ntt_rns_mod_down_add_batch, TRANSFORMED | ACCUMULATE, at the same shape                          -- the PARENT commit's library
  (the parent's library is LIB, built by tools/build_head.sh, selected with NTT_LIB)

24 Q limbs of 50-bit primes, np = 1 / 2 / 4 / 8 P limbs of 60-bit primes, N = 2^13 and 2^14, 2 / 64 / 1024 polynomials.  torch is imported
first, so the library binds to the HIP runtime torch loaded; every call goes to ONE torch stream.  The two libraries run in ALTERNATING
child processes on the same board, round by round; inside a child the variants of a shape are timed INTERLEAVED, three windows each in
an order that rotates from round to round, and a variant's figure for the round is the median of its windows.  Printed per shape: the
median ms per call of each variant, the parent's own run-to-run spread over the rounds (max / min of its figure) and the call-rate ratios
as RANGES over the rounds."""
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
NPS = (2,) if a.quick else (1, 2, 4, 8)
BATCHES = (2, 64) if a.quick else (2, 64, 1024)
TMOD = 65537
T, ACC = 1, 4


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(which, logn, rnd):
    """every shape once: {"form,np,batch,variant": ms per call} as one JSON line"""
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
    ct = torch.empty(NL * top * n, dtype=torch.int64, device="cuda:0")
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
            if l < NL:
                lib.fill_uniform(ct.data_ptr() + 8 * l * per, per, q, 177 + l, 0, stream=sp)
        st.synchronize()
        for np_ in NPS:
            # the P limbs follow the Q limbs in the buffer: [NL + np][batch][N]
            ps = plans[:NL] + plans[NL:NL + np_]
            if which == "prev":
                down = {"down0": lambda: lib.rns_mod_down(ps, np_, buf.data_ptr(), batch, T, stream=sp)}
                add = {"add0": lambda: lib.rns_mod_down_add(ps, np_, ct.data_ptr(), buf.data_ptr(), batch, T | ACC, stream=sp)}
            else:
                def call(opt, form):
                    def f():
                        plans[0].set_option(lib.OPT_BGV_FUSED, opt)
                        if form == "down":
                            lib.rns_mod_down_bgv(ps, np_, buf.data_ptr(), TMOD, batch, T, stream=sp)
                        else:
                            lib.rns_mod_down_bgv_add(ps, np_, ct.data_ptr(), buf.data_ptr(), TMOD, batch, T | ACC, stream=sp)
                    return f
                down = {"fused": call(1, "down"), "sand": call(0, "down")}
                add = {"fused": call(1, "add"), "sand": call(0, "add")}
            for form, fns in (("down", down), ("add", add)):
                for name, ms in interleaved(fns).items():
                    out["%s,%d,%d,%s" % (form, np_, batch, name)] = ms
        if which != "prev":
            plans[0].set_option(lib.OPT_BGV_FUSED, -1)
    print(json.dumps(out))


def rng(xs):
    return "%.2f..%.2f" % (min(xs), max(xs))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/bgv_bench.py  library sha256 %s" % sha(cur))
    print("# parent library %s sha256 %s" % (os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("# %d Q limbs of 50-bit primes, np 60-bit P primes, T = %d, NTT domain; %d rounds of alternating child processes, each timing the" % (NL, TMOD, ROUNDS))
    print("# variants of a shape interleaved, %d windows each, in an order rotated by the round; %d calls after %d warm-up calls per window;" % (WINDOWS, CALLS, WARM))
    print("# ms = median over the rounds; ratios = call rates, min..max over the rounds; spread = max / min of the parent's figure")
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
        for form, base, what in (("down", "down0", "parent ModDown    "), ("add", "add0", "parent ModDown-add")):
            for batch in BATCHES:
                for np_ in NPS:
                    k = "%s,%d,%d," % (form, np_, batch)
                    p, f, s = col("prev", k + base), col("cur", k + "fused"), col("cur", k + "sand")
                    print("%-4s N=2^%d polys=%-5d np=%d  %s %8.4f ms (spread %.2f)  fused %8.4f ms  sandwich %8.4f ms  sandwich/fused %s  "
                          "parent/fused %s  parent/sandwich %s" % (form, logn, batch, np_, what, med(p), max(p) / min(p), med(f), med(s),
                                                                   rng([x / y for x, y in zip(s, f)]), rng([x / y for x, y in zip(p, f)]),
                                                                   rng([x / y for x, y in zip(p, s)])))
                sys.stdout.flush()


if a.child:
    child(a.child[0], int(a.child[1]), int(a.child[2]))
else:
    main()
