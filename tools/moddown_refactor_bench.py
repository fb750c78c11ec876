#!/usr/bin/env python3
"""tools/moddown_refactor_bench.py [--quick] [--prev LIB] [--logn 13 14] [--rounds R]: the fused routes of the four kernels that share
moddown_fwd_body (csrc/ntt_kernels_moddown.h), the parent commit's library (LIB, built by tools/build_head.sh, selected with NTT_LIB)
against this tree's, on the method of profiles/r13/refactor_bench.txt:

  moddown   ntt_rns_mod_down_batch, NTT_OPT_RESCALE_FUSED 1                                   (moddown_fwd_kernel)
  add       ntt_rns_mod_down_add_batch, ACCUMULATE, NTT_OPT_MODDOWN_ADD_FUSED 1               (ksfold_fwd_kernel)
  bgv       ntt_rns_mod_down_bgv_batch, T = 65537, NTT_OPT_BGV_FUSED 1                        (moddown_bgv_fwd_kernel, in place)
  bgv_add   ntt_rns_mod_down_bgv_add_batch, ACCUMULATE, T = 65537, NTT_OPT_BGV_FUSED 1        (moddown_bgv_fwd_kernel, into a ciphertext)
  exact     ntt_rns_mod_down_exact_batch, mult = 65537, NTT_OPT_RESCALE_FUSED 1               (moddown_exact_fwd_kernel)

All TRANSFORMED, 16 Q limbs of 50-bit primes, np = 1 (50-bit), 2, 4 (60-bit) P primes, N = 2^13 and 2^14, 64 and 1024 polynomials.  BOTH
children issue the same calls, so each library gives a time for every shape.  Device events, windows of 10 calls after 3 warm-up calls, 3
windows per shape with the shapes of a batch size interleaved in an order rotated by the round, a child's figure = the median of its
windows; the two libraries in ALTERNATING child processes (parent, tree, parent, ...).  Pass condition per shape: the tree's range
overlaps the parent's, or the tree's slowest round is no further from the parent's median than the parent's own slowest-to-fastest
spread in this run."""
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
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--child", nargs=3, metavar=("WHICH", "LOGN", "ROUND"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM, WINDOWS = (2, 3, 2, 2) if a.quick else (a.rounds, 10, 3, 3)
NQ = 16
NPS = (2,) if a.quick else (1, 2, 4)
BATCHES = (64,) if a.quick else (64, 1024)
TMOD = 65537
T, ACC = 1, 4
FORMS = ("moddown", "add", "bgv", "bgv_add", "exact")


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def child(logn, rnd):
    """every shape once: {"form,np,batch": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    n = 1 << logn
    qs = [lib.find_prime(50, n, k) for k in range(NQ)]
    p50 = lib.find_prime(50, n, NQ)
    p60 = [lib.find_prime(60, n, k) for k in range(max(NPS))]
    plan = lambda q: lib.Plan(n, q, lib.min_root(q, n))
    qplans, p50plan, p60plans = [plan(q) for q in qs], plan(p50), [plan(q) for q in p60]
    for opt in (lib.OPT_RESCALE_FUSED, lib.OPT_MODDOWN_ADD_FUSED, lib.OPT_BGV_FUSED):
        qplans[0].set_option(opt, 1)
    top = max(BATCHES)
    st = torch.cuda.Stream(device=0)
    sp = st.cuda_stream
    # one accumulator per kind of P prime (the P limbs are inverse-transformed in place by every call), [NQ + np][batch][N]
    bufs = {1: torch.empty((NQ + 1) * top * n, dtype=torch.int64, device="cuda:0"),
            60: torch.empty((NQ + max(NPS)) * top * n, dtype=torch.int64, device="cuda:0")}
    ct = torch.empty(NQ * top * n, dtype=torch.int64, device="cuda:0")
    low = min(qs + [p50])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        with torch.cuda.stream(st):
            e0.record(st)
            for _ in range(CALLS):
                fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS

    out = {}
    for batch in BATCHES:
        per = batch * n
        # canonical words in every slot (they stay canonical under every call timed here); the P slots start below every prime
        for buf in bufs.values():
            for l in range(buf.numel() // (top * n)):
                lib.fill_uniform(buf.data_ptr() + 8 * l * per, per, qs[l] if l < NQ else low, 77 + l, 0, stream=sp)
        for l in range(NQ):
            lib.fill_uniform(ct.data_ptr() + 8 * l * per, per, qs[l], 177 + l, 0, stream=sp)
        st.synchronize()
        fns = {}
        for np_ in NPS:
            ps = qplans + ([p50plan] if np_ == 1 else p60plans[:np_])
            b, c = bufs[1 if np_ == 1 else 60].data_ptr(), ct.data_ptr()
            fns["moddown,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down(ps, np_, b, batch, T, stream=sp)
            fns["add,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_add(ps, np_, c, b, batch, T | ACC, stream=sp)
            fns["bgv,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_bgv(ps, np_, b, TMOD, batch, T, stream=sp)
            fns["bgv_add,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_bgv_add(ps, np_, c, b, TMOD, batch, T | ACC, stream=sp)
            fns["exact,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_exact(ps, np_, b, TMOD, batch, T, stream=sp)
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
        for name in names:
            out[name] = statistics.median(t[name])
    print(json.dumps(out))


def main():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    print("# tools/moddown_refactor_bench.py")
    print("# tree library   sha256 %s" % sha(cur))
    print("# parent library sha256 %s (%s)" % (sha(a.prev), os.path.relpath(a.prev, ROOT)))
    print("# %d rounds of alternating child processes (parent, tree, ...); ms per call, min..max over the rounds" % ROUNDS)
    outside, ratios, shapes = 0, [], 0
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
            for np_ in NPS:
                for form in FORMS:
                    k = "%s,%d,%d" % (form, np_, batch)
                    p, t = [r[k] for r in rounds["prev"]], [r[k] for r in rounds["cur"]]
                    pm, tm = statistics.median(p), statistics.median(t)
                    overlap = min(t) <= max(p) and min(p) <= max(t)
                    near = max(t) - pm <= max(p) - min(p)
                    verdict = "pass (ranges overlap)" if overlap else "pass (within the parent's spread)" if near else "OUTSIDE"
                    outside += verdict == "OUTSIDE"
                    shapes += 1
                    ratios.append(tm / pm)
                    print("%-8s np=%d N=2^%d polys=%-5d parent %8.4f..%8.4f (median %8.4f)  tree %8.4f..%8.4f (median %8.4f)  tree/parent median %.3f  %s"
                          % (form, np_, logn, batch, min(p), max(p), pm, min(t), max(t), tm, tm / pm, verdict))
                    sys.stdout.flush()
    print("# %d shapes, %d outside the pass condition; tree / parent medians %.3f .. %.3f" % (shapes, outside, min(ratios), max(ratios)))


if a.child:
    child(int(a.child[1]), int(a.child[2]))
else:
    main()
