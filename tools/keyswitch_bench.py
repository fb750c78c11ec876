#!/usr/bin/env python3
"""tools/keyswitch_bench.py [--quick] [--prev LIB]: ModDown / ModUp (ntt_rns_mod_down_batch, ntt_rns_mod_up_batch) timed with device
events after warm-ups.

(1) the gate: NTT-domain ModDown with np = 1 against the parent commit's ntt_rns_rescale_batch (LIB, built by tools/build_head.sh,
    selected with NTT_LIB) at N = 2^14 over the same 17 50-bit primes (the rescale drops the last one; ModDown takes nq = 16,
    np = 1), round, 2 / 64 / 1024 polynomials.  The two calls run in ALTERNATING child processes on the same box, round by round;
    printed per batch: the median ms per call of each and the call-rate ratio (pass mark 0.90).
(2) NTT-domain ModDown with np = 2 and 4 (16 50-bit Q primes, 60-bit P primes): the fused route and the sandwich alternating in one
    process; the fraction of 8 TB/s at the fused route's 8N(2nq + 3np) bytes per polynomial.
(3) coefficient ModUp at (count, nlimbs) = (2, 10), (4, 20), (12, 40), N = 2^16, 64 polynomials: its rate as a fraction of
    ntt_copy_probe moving the same bytes (count words read per launch of 16 destinations, one word written per destination) in the
    same process.
Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer rounds (a smoke run of the tool)")
ap.add_argument("--prev", default=os.path.join(ROOT, "build", "libntt_prev.so"), help="the parent commit's library")
ap.add_argument("--child", nargs=2, metavar=("CALL", "BATCH"), help=argparse.SUPPRESS)
a = ap.parse_args()
ROUNDS, CALLS, WARM = (2, 3, 2) if a.quick else (7, 10, 5)

import ontt  # noqa: E402  (after NTT_LIB is in place for a child)

lib = ontt.load()


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def make(n, bits):
    seen, plans = {}, []
    for b in bits:
        k = seen.get(b, 0)
        seen[b] = k + 1
        q = lib.find_prime(b, n, k)
        plans.append(lib.Plan(n, q, lib.min_root(q, n)))
    return plans


def fill(buf, plans, n, batch):
    per = batch * n
    for l, p in enumerate(plans):
        lib.fill_uniform(buf.ptr + 8 * l * per, per, p.q, 77 + l, 0)
    lib.stream_sync()


def time_calls(fn):
    e0, e1 = lib.Event(), lib.Event()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    lib.stream_sync()
    return e1.elapsed_ms_since(e0) / CALLS


def child(call, batch):
    """one gate measurement: median ms per call over ROUNDS rounds of CALLS calls after WARM warm-ups"""
    n = 1 << 14
    plans = make(n, [50] * 17)
    buf = lib.DeviceBuffer(17 * batch * n)
    fill(buf, plans, n, batch)
    if call == "rescale":
        fn = lambda: lib.rns_rescale(plans, buf.ptr, batch, lib.RESCALE_TRANSFORMED)  # noqa: E731
    else:
        fn = lambda: lib.rns_mod_down(plans, 1, buf.ptr, batch, lib.MODDOWN_TRANSFORMED)  # noqa: E731
    for _ in range(WARM):
        fn()
    lib.stream_sync()
    print("%.6f" % statistics.median(time_calls(fn) for _ in range(ROUNDS)))
    buf.free()
    for p in plans:
        p.destroy()


def gate():
    print("# (1) gate: NTT-domain ModDown (np = 1, this library) against the parent's ntt_rns_rescale_batch (%s, sha256 %s)" % (
        os.path.relpath(a.prev, ROOT), sha(a.prev)))
    print("#     N = 2^14, 17 x 50-bit primes, round; alternating child processes, %d rounds; ms per call = median over the rounds" % ROUNDS)
    worst = None
    for batch in (2, 64, 1024):
        times = {"rescale": [], "moddown": []}
        for _ in range(ROUNDS):
            for call in ("rescale", "moddown"):
                env = dict(os.environ)
                if call == "rescale":
                    env["NTT_LIB"] = a.prev
                else:
                    env.pop("NTT_LIB", None)
                args = [sys.executable, os.path.abspath(__file__), "--child", call, str(batch)] + (["--quick"] if a.quick else [])
                out = subprocess.run(args, env=env, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    raise SystemExit("child %s %d failed (%d): %s" % (call, batch, out.returncode, out.stderr[-2000:]))
                times[call].append(float(out.stdout.split()[-1]))
        mr, mm = statistics.median(times["rescale"]), statistics.median(times["moddown"])
        ratio = mr / mm
        worst = ratio if worst is None else min(worst, ratio)
        print("gate  N=2^14 L+1=17 batch=%-5d  parent rescale %8.4f ms  moddown np=1 %8.4f ms  call rate moddown / rescale %.3f  %s" % (
            batch, mr, mm, ratio, "PASS" if ratio >= 0.90 else "FAIL"))
    print("gate  worst ratio %.3f (pass mark 0.90): %s" % (worst, "PASS" if worst >= 0.90 else "FAIL"))


def moddown_routes():
    print("# (2) NTT-domain ModDown, 16 x 50-bit Q primes, np x 60-bit P primes: fused and sandwich alternating in one process;")
    print("#     bytes = the fused route's 8N(2nq + 3np) per polynomial")
    n, nq = 1 << 14, 16
    for np_ in (2, 4):
        for batch in (2, 64, 1024):
            plans = make(n, [50] * nq + [60] * np_)
            buf = lib.DeviceBuffer((nq + np_) * batch * n)
            fill(buf, plans, n, batch)
            fn = lambda: lib.rns_mod_down(plans, np_, buf.ptr, batch, lib.MODDOWN_TRANSFORMED)  # noqa: E731
            for fused in (1, 0):
                plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
                for _ in range(WARM):
                    fn()
            lib.stream_sync()
            times = {1: [], 0: []}
            for _ in range(ROUNDS):
                for fused in (1, 0):
                    plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
                    times[fused].append(time_calls(fn))
            med = {r: statistics.median(v) for r, v in times.items()}
            nbytes = 8 * n * batch * (2 * nq + 3 * np_)
            print("moddown  N=2^14 nq=%d np=%d batch=%-5d fused %8.4f ms (%.3f of 8 TB/s)  sandwich %8.4f ms  fused / sandwich call rate %.2f x" % (
                nq, np_, batch, med[1], nbytes / (med[1] * 1e-3) / PEAK, med[0], med[0] / med[1]))
            buf.free()
            for p in plans:
                p.destroy()


def modup():
    print("# (3) coefficient ModUp, N = 2^16, 64 polynomials, 50-bit primes (a 60-bit first prime): rate against ntt_copy_probe of the")
    print("#     same bytes (count words read per launch of up to 16 destination limbs, one word written per destination limb)")
    n, batch = 1 << 16, 64
    for count, nl in ((2, 10), (4, 20), (12, 40)):
        plans = make(n, [60] + [50] * (nl - 1))
        buf = lib.DeviceBuffer(nl * batch * n)
        fill(buf, plans, n, batch)
        ndst = nl - count
        launches = (ndst + 15) // 16
        words = batch * n * (count * launches + ndst)
        src, dst = lib.DeviceBuffer(words // 2), lib.DeviceBuffer(words // 2)
        up = lambda: lib.rns_mod_up(plans, buf.ptr, 0, count, batch, 0)  # noqa: E731
        cp = lambda: lib.copy_probe(dst.ptr, src.ptr, words // 2)  # noqa: E731  (16 bytes per copied word pair: 8 * words in all)
        for _ in range(WARM):
            up(), cp()
        lib.stream_sync()
        t_up, t_cp = [], []
        for _ in range(ROUNDS):
            t_up.append(time_calls(up))
            t_cp.append(time_calls(cp))
        mu, mc = statistics.median(t_up), statistics.median(t_cp)
        print("modup  N=2^16 batch=%d count=%-2d nlimbs=%-2d  %8.4f ms  %8.1f MB  %.3f of 8 TB/s  copy_probe %8.4f ms  modup / copy rate %.2f" % (
            batch, count, nl, mu, 8 * words / 1e6, 8 * words / (mu * 1e-3) / PEAK, mc, mc / mu))
        for b in (buf, src, dst):
            b.free()
        for p in plans:
            p.destroy()


if a.child:
    child(a.child[0], int(a.child[1]))
    sys.exit(0)
print("# tools/keyswitch_bench.py  library sha256 %s  HIP %s" % (sha(lib.LIB_PATH), lib.version()))
print("# %d rounds x %d calls after %d warm-up calls" % (ROUNDS, CALLS, WARM))
gate()
moddown_routes()
modup()
