#!/usr/bin/env python3
"""tools/rescale_bench.py [--quick]: the RNS rescale (ntt_rns_rescale_batch) timed with device events after warm-ups.

NTT domain: the fused route (rescale_fwd_kernel, NTT_OPT_RESCALE_FUSED 1) and the sandwich (inverse / element-wise / forward,
NTT_OPT_RESCALE_FUSED 0) alternate in one process, round by round, at N = 2^12, 2^13, 2^14 with L+1 = 5 and 17 limbs of 50-bit
primes and 2, 64, 1024 polynomials (operands capped at 3 GB); the sandwich alone at 2^16; the coefficient form at 2^14 and 2^16.
Printed per case: ms per call (median of the rounds), the algorithmic bytes of the route -- fused 8N(2L+3), sandwich 8N(6L+3),
coefficients 8N(2L+1) per polynomial -- and that rate as a fraction of 8 TB/s.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ontt

lib = ontt.load()
PEAK = 8e12
CAP_BYTES = 3 << 30

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer rounds (a smoke run of the tool)")
a = ap.parse_args()
ROUNDS, CALLS, WARM = (2, 3, 2) if a.quick else (7, 10, 5)


def lib_sha():
    with open(lib.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def make(n, nl):
    qs = [lib.find_prime(50, n, i) for i in range(nl)]
    return [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]


def fill(buf, plans, n, batch):
    per = batch * n
    for l, p in enumerate(plans):
        lib.fill_uniform(buf.ptr + 8 * l * per, per, p.q, 77 + l, 0)
    lib.stream_sync()


def time_calls(plans, buf, batch, flags):
    e0, e1 = lib.Event(), lib.Event()
    e0.record()
    for _ in range(CALLS):
        lib.rns_rescale(plans, buf.ptr, batch, flags)
    e1.record()
    lib.stream_sync()
    return e1.elapsed_ms_since(e0) / CALLS


def report(tag, n, nl, batch, route, ms, words_per_poly):
    nbytes = 8 * words_per_poly * n * batch
    print("%-12s N=2^%-2d L+1=%-2d batch=%-5d %-9s %9.4f ms/call  %8.1f MB  %.3f of 8 TB/s" % (
        tag, n.bit_length() - 1, nl, batch, route, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / PEAK))


def case(n, nl, batch, routes, flags):
    if 8 * n * nl * batch > CAP_BYTES:
        return
    plans = make(n, nl)
    buf = lib.DeviceBuffer(nl * batch * n)
    fill(buf, plans, n, batch)
    L = nl - 1
    for fused in routes:
        plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
        for _ in range(WARM):
            lib.rns_rescale(plans, buf.ptr, batch, flags)
    lib.stream_sync()
    times = {r: [] for r in routes}
    for _ in range(ROUNDS):  # the routes alternate, round by round
        for fused in routes:
            plans[0].set_option(lib.OPT_RESCALE_FUSED, fused)
            times[fused].append(time_calls(plans, buf, batch, flags))
    med = {r: statistics.median(v) for r, v in times.items()}
    if flags & lib.RESCALE_TRANSFORMED:
        for fused in routes:
            report("ntt-domain", n, nl, batch, "fused" if fused else "sandwich", med[fused], (2 * L + 3) if fused else (6 * L + 3))
        if len(routes) == 2:
            print("%-12s N=2^%-2d L+1=%-2d batch=%-5d fused / sandwich call rate: %.2f x" % (
                "", n.bit_length() - 1, nl, batch, med[0] / med[1]))
    else:
        report("coefficient", n, nl, batch, "coef", med[routes[0]], 2 * L + 1)
    buf.free()
    for p in plans:
        p.destroy()


print("# tools/rescale_bench.py  library sha256 %s  HIP %s" % (lib_sha(), lib.version()))
print("# %d rounds x %d calls after %d warm-up calls per route; ms per call = median over the rounds" % (ROUNDS, CALLS, WARM))
for logn in (12, 13, 14):
    for nl in (5, 17):
        for batch in (2, 64, 1024):
            case(1 << logn, nl, batch, (1, 0), lib.RESCALE_TRANSFORMED)
for nl in (5, 17):
    for batch in (2, 64):
        case(1 << 16, nl, batch, (0,), lib.RESCALE_TRANSFORMED)
for logn in (14, 16):
    for nl in (5, 17):
        for batch in (64, 256):
            case(1 << logn, nl, batch, (1,), 0)
