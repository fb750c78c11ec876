#!/usr/bin/env python3
"""tools/moddown_refactor_bench.py [--set moddown|produce] [--quick] [--prev LIB] [--logn 13 14] [--rounds R]: a refactored kernel family's
calls, the parent commit's library (LIB, built by tools/build_head.sh, selected with NTT_LIB) against this tree's, on the method of
profiles/r13/refactor_bench.txt.

--set moddown (the default): the fused routes of the four kernels that share moddown_fwd_body (csrc/ntt_kernels_moddown.h):

  moddown   ntt_rns_mod_down_batch, NTT_OPT_RESCALE_FUSED 1                                   (moddown_fwd_kernel)
  add       ntt_rns_mod_down_add_batch, ACCUMULATE, NTT_OPT_MODDOWN_ADD_FUSED 1               (ksfold_fwd_kernel)
  bgv       ntt_rns_mod_down_bgv_batch, T = 65537, NTT_OPT_BGV_FUSED 1                        (moddown_bgv_fwd_kernel, in place)
  bgv_add   ntt_rns_mod_down_bgv_add_batch, ACCUMULATE, T = 65537, NTT_OPT_BGV_FUSED 1        (moddown_bgv_fwd_kernel, into a ciphertext)
  exact     ntt_rns_mod_down_exact_batch, mult = 65537, NTT_OPT_RESCALE_FUSED 1               (moddown_exact_fwd_kernel)

All TRANSFORMED, 16 Q limbs of 50-bit primes, np = 1 (50-bit), 2, 4 (60-bit) P primes, N = 2^13 and 2^14, 64 and 1024 polynomials.

--set produce: the kernels that share produce_fwd_body (csrc/ntt_kernels_produce.h) and the coefficient kernels beside them, behind
produce_route (csrc/host/host_produce.inc):

  lift.MODE.store / .acc      ntt_rns_from_plain_batch (centred, scaled) / ntt_rns_from_double_batch, TRANSFORMED (| ACCUMULATE),
                              NTT_OPT_LIFT_FUSED 1                                                       (lift_fwd_kernel)
  sample.KIND.store / .acc    ntt_rns_sample_batch (ternary, cbd21), TRANSFORMED (| ACCUMULATE), NTT_OPT_SAMPLE_FUSED 1
                                                                                                         (sample_fwd_kernel)
  lift.MODE.coef              the lifts without TRANSFORMED, storing                                     (lift_coef_kernel)
  sample.KIND.coef            the sampler (ternary, cbd21, uniform) without TRANSFORMED, storing         (sample_coef_kernel)

L = 1, 4, 16 limbs of 50-bit primes, t = 65537, N = 2^13 and 2^14, 64 and 1024 polynomials.

BOTH children issue the same calls, so each library gives a time for every shape.  Device events, windows of 10 calls after 3 warm-up calls, 3
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
ap.add_argument("--set", choices=("moddown", "produce"), default="moddown", help="the family of calls")
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
FORMS = ("moddown", "add", "bgv", "bgv_add", "exact")  # (the order of the moddown set's report)
LS = (1, 4) if a.quick else (1, 4, 16)


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def moddown_calls(lib, torch, n, st):
    """per batch size: {"form,np,batch": the call}"""
    sp = st.cuda_stream
    qs = [lib.find_prime(50, n, k) for k in range(NQ)]
    p50 = lib.find_prime(50, n, NQ)
    p60 = [lib.find_prime(60, n, k) for k in range(max(NPS))]
    plan = lambda q: lib.Plan(n, q, lib.min_root(q, n))
    qplans, p50plan, p60plans = [plan(q) for q in qs], plan(p50), [plan(q) for q in p60]
    for opt in (lib.OPT_RESCALE_FUSED, lib.OPT_MODDOWN_ADD_FUSED, lib.OPT_BGV_FUSED):
        qplans[0].set_option(opt, 1)
    top = max(BATCHES)
    # one accumulator per kind of P prime (the P limbs are inverse-transformed in place by every call), [NQ + np][batch][N]
    bufs = {1: torch.empty((NQ + 1) * top * n, dtype=torch.int64, device="cuda:0"),
            60: torch.empty((NQ + max(NPS)) * top * n, dtype=torch.int64, device="cuda:0")}
    ct = torch.empty(NQ * top * n, dtype=torch.int64, device="cuda:0")
    low = min(qs + [p50])
    for batch in BATCHES:
        per = batch * n
        # canonical words in every slot (they stay canonical under every call timed here); the P slots start below every prime
        for buf in bufs.values():
            for l in range(buf.numel() // (top * n)):
                lib.fill_uniform(buf.data_ptr() + 8 * l * per, per, qs[l] if l < NQ else low, 77 + l, 0, stream=sp)
        for l in range(NQ):
            lib.fill_uniform(ct.data_ptr() + 8 * l * per, per, qs[l], 177 + l, 0, stream=sp)
        fns = {}
        for np_ in NPS:
            ps = qplans + ([p50plan] if np_ == 1 else p60plans[:np_])
            b, c = bufs[1 if np_ == 1 else 60].data_ptr(), ct.data_ptr()
            fns["moddown,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down(ps, np_, b, batch, T, stream=sp)
            fns["add,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_add(ps, np_, c, b, batch, T | ACC, stream=sp)
            fns["bgv,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_bgv(ps, np_, b, TMOD, batch, T, stream=sp)
            fns["bgv_add,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_bgv_add(ps, np_, c, b, TMOD, batch, T | ACC, stream=sp)
            fns["exact,%d,%d" % (np_, batch)] = lambda ps=ps, np_=np_, b=b: lib.rns_mod_down_exact(ps, np_, b, TMOD, batch, T, stream=sp)
        yield fns


def produce_calls(lib, torch, n, st):
    """per batch size: {"form,L,batch": the call}"""
    sp = st.cuda_stream
    top_l, top = max(LS), max(BATCHES)
    qs = [lib.find_prime(50, n, k) for k in range(top_l)]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    plans[0].set_option(lib.OPT_LIFT_FUSED, 1)
    plans[0].set_option(lib.OPT_SAMPLE_FUSED, 1)
    # the output's limbs, then the plaintext words, then the doubles
    pool = torch.empty((top_l + 2) * top * n, dtype=torch.int64, device="cuda:0")
    c, m_off = pool.data_ptr(), top_l * top * n
    dm, dy = c + 8 * m_off, c + 8 * (m_off + top * n)
    SCALE, TR, ACC = 1, 2, 4  # (NTT_LIFT_* and NTT_SAMPLE_*: the same values)
    kinds = (("ternary", lib.SAMPLE_TERNARY), ("cbd21", lib.SAMPLE_CBD21), ("uniform", lib.SAMPLE_UNIFORM))
    for batch in BATCHES:
        per = batch * n
        lib.fill_uniform(dm, per, TMOD, 5, 0, stream=sp)
        with torch.cuda.stream(st):
            pool[m_off + top * n:m_off + top * n + per].view(torch.float64).copy_((pool[m_off:m_off + per] - TMOD // 2).to(torch.float64) / 64.0)
        # canonical words in every limb (they stay canonical under every call timed here)
        for l in range(top_l):
            lib.fill_uniform(c + 8 * l * per, per, qs[l], 77 + l, 0, stream=sp)
        fns = {}
        for nl in LS:
            ps = plans[:nl]
            for tag, fl in (("store", TR), ("acc", TR | ACC), ("coef", 0)):
                k = lambda form: "%s.%s,%d,%d" % (form, tag, nl, batch)
                fns[k("lift.centred")] = lambda ps=ps, fl=fl: lib.rns_from_plain(ps, c, dm, TMOD, batch, fl, stream=sp)
                fns[k("lift.scaled")] = lambda ps=ps, fl=fl: lib.rns_from_plain(ps, c, dm, TMOD, batch, fl | SCALE, stream=sp)
                fns[k("lift.double")] = lambda ps=ps, fl=fl: lib.rns_from_double(ps, c, dy, 2.0 ** 30, batch, fl, stream=sp)
                for name, kind in kinds[:2 if fl else 3]:
                    fns[k("sample." + name)] = lambda ps=ps, fl=fl, kind=kind: lib.rns_sample(ps, c, kind, 0x5EED, batch, flags=fl, stream=sp)
        yield fns


def child(logn, rnd):
    """every shape once: {"form,np or L,batch": ms per call} as one JSON line"""
    import torch  # (first: the library binds to the HIP runtime torch loaded)
    torch.cuda.set_device(0)
    import ontt  # (after NTT_LIB is in place)
    lib = ontt.load()
    st = torch.cuda.Stream(device=0)
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
    for fns in (moddown_calls if a.set == "moddown" else produce_calls)(lib, torch, 1 << logn, st):
        st.synchronize()
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
    print("# tools/moddown_refactor_bench.py --set %s" % a.set)
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
                args = [sys.executable, os.path.abspath(__file__), "--set", a.set, "--child", which, str(logn), str(rnd)] + (["--quick"] if a.quick else [])
                r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("child %s 2^%d failed (%d): %s" % (which, logn, r.returncode, r.stderr[-2000:]))
                rounds[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
        order = lambda k: (int(k.split(",")[2]), int(k.split(",")[1]), FORMS.index(k.split(",")[0]) if a.set == "moddown" else k)
        width = max(len(k.split(",")[0]) for k in rounds["cur"][0])
        for k in sorted(rounds["cur"][0], key=order):
            form, np_, batch = k.split(",")[0], int(k.split(",")[1]), int(k.split(",")[2])
            p, t = [r[k] for r in rounds["prev"]], [r[k] for r in rounds["cur"]]
            pm, tm = statistics.median(p), statistics.median(t)
            overlap = min(t) <= max(p) and min(p) <= max(t)
            near = max(t) - pm <= max(p) - min(p)
            verdict = "pass (ranges overlap)" if overlap else "pass (within the parent's spread)" if near else "OUTSIDE"
            outside += verdict == "OUTSIDE"
            shapes += 1
            ratios.append(tm / pm)
            print("%-*s %s=%d N=2^%d polys=%-5d parent %8.4f..%8.4f (median %8.4f)  tree %8.4f..%8.4f (median %8.4f)  tree/parent median %.3f  %s"
                  % (max(8, width), form, "np" if a.set == "moddown" else "L", np_, logn, batch, min(p), max(p), pm, min(t), max(t), tm, tm / pm, verdict))
            sys.stdout.flush()
    print("# %d shapes, %d outside the pass condition; tree / parent medians %.3f .. %.3f" % (shapes, outside, min(ratios), max(ratios)))


if a.child:
    child(int(a.child[1]), int(a.child[2]))
else:
    main()
