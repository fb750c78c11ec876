#!/usr/bin/env python3
"""tools/galois_bench.py [--quick] [--out FILE]: the Galois automorphisms and the rotation key product (ntt_rns_galois_batch,
ntt_rns_galois_dot_batch) timed with device events after warm-ups; every shape alternates, in one process, with ntt_copy_probe
moving the same number of bytes.  Writes FILE (default profiles/r09/galois_bench.txt) and prints it.

(1) the automorphism, 17 limbs (a 60-bit prime and 16 50-bit ones: two launches), N = 2^14 and 2^16, 2 / 64 / 1024 polynomials:
    NTT domain with 16-byte accesses (galois_ntt_kernel<true>), NTT domain with 8-byte accesses (the same call on buffers 8 bytes
    off the 16-byte grid: galois_ntt_kernel<false>) and coefficients (galois_coef_kernel), each at 16N bytes per limb and polynomial.
(2) the rotation key product, 17 limbs, k = 3 and 8, with a key per polynomial (8N(2k + 1) bytes per limb and polynomial) and with
    a broadcast key (8N(k + 1)); ns per product word beside the rate, to compare the forms at equal products.
Per row: ms per call (median over the rounds), bytes/s at the algorithmic bytes, the copy probe's bytes/s, their ratio.
Kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer rounds and the small shapes only (a smoke run of the tool)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "galois_bench.txt"))
a = ap.parse_args()
ROUNDS, CALLS, WARM = (2, 3, 2) if a.quick else (7, 10, 5)

import ontt  # noqa: E402

lib = ontt.load()
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def time_calls(fn):
    e0, e1 = lib.Event(), lib.Event()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    lib.stream_sync()
    return e1.elapsed_ms_since(e0) / CALLS


def against_copy(fn, nbytes, cdst, csrc):
    """(median ms of fn, median ms of a copy probe moving nbytes), the two alternating round by round"""
    cp = lambda: lib.copy_probe(cdst, csrc, nbytes // 16)  # noqa: E731  (n words copied: 8n read + 8n written)
    for _ in range(WARM):
        fn(), cp()
    lib.stream_sync()
    tf, tc = [], []
    for _ in range(ROUNDS):
        tf.append(time_calls(fn))
        tc.append(time_calls(cp))
    return statistics.median(tf), statistics.median(tc)


def row(tag, desc, ms, mc, nbytes, extra=""):
    say("%-8s %-44s %9.4f ms  %8.1f MB  %6.3f TB/s  copy_probe %9.4f ms %6.3f TB/s  ratio %.2f%s" % (
        tag, desc, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, mc, nbytes / (mc * 1e-3) / 1e12, mc / ms, extra))


BITS = [60] + [50] * 16


def automorphism():
    say("# (1) sigma_g, 17 limbs, g = 5^3 mod 2N, out of place: 16N bytes per limb and polynomial")
    for logn in (14, 16):
        n = 1 << logn
        plans = make(n, BITS)
        g = lib.galois_rotation(n, 3)
        for batch in ((2, 64) if a.quick else (2, 64, 1024)):
            words = len(plans) * batch * n
            src, dst = lib.DeviceBuffer(words + 2), lib.DeviceBuffer(words + 2)
            nbytes = 16 * words
            for tag, flags, off in (("ntt16", lib.GALOIS_TRANSFORMED, 0), ("ntt8", lib.GALOIS_TRANSFORMED, 8), ("coef", 0, 0)):
                fn = lambda: lib.rns_galois(plans, dst.ptr + off, src.ptr + off, g, batch, flags)  # noqa: E731
                ms, mc = against_copy(fn, nbytes, dst.ptr, src.ptr)
                row(tag, "N=2^%d limbs=17 batch=%d" % (logn, batch), ms, mc, nbytes)
            src.free(), dst.free()
        for p in plans:
            p.destroy()


def key_product():
    say("# (2) c^ = sum_{i<k} sigma_g(a_i^) (.) key_i^, 17 limbs, g = 5^3 mod 2N: 8N(2k + 1) bytes per limb and polynomial, 8N(k + 1) with")
    say("#     a broadcast key (the key's own N words per limb not counted)")
    shapes = [(14, 64)] if a.quick else [(14, 2), (14, 64), (14, 1024), (16, 64)]
    for logn, batch in shapes:
        n = 1 << logn
        plans = make(n, BITS)
        g = lib.galois_rotation(n, 3)
        words = len(plans) * batch * n
        for k in (3, 8):
            av = [lib.DeviceBuffer(words) for _ in range(k)]
            kv = [lib.DeviceBuffer(words) for _ in range(k)]
            c = lib.DeviceBuffer(words)
            for bc in (0, lib.GALOIS_KEY_BROADCAST):
                nbytes = 8 * words * ((k + 1) if bc else (2 * k + 1))
                cs, cd = lib.DeviceBuffer(nbytes // 16), lib.DeviceBuffer(nbytes // 16)
                fn = lambda: lib.rns_galois_dot(plans, c.ptr, [x.ptr for x in av], [x.ptr for x in kv], g, batch, lib.GALOIS_TRANSFORMED | bc)  # noqa: E731
                ms, mc = against_copy(fn, nbytes, cd.ptr, cs.ptr)
                row("dot", "N=2^%d limbs=17 batch=%d k=%d %s" % (logn, batch, k, "broadcast key" if bc else "key per polynomial"), ms, mc, nbytes,
                    "  %.4f ns per product word" % (ms * 1e6 / (k * words)))
                cs.free(), cd.free()
            for b in av + kv + [c]:
                b.free()
        for p in plans:
            p.destroy()


say("# tools/galois_bench.py  library sha256 %s  HIP %s" % (sha(lib.LIB_PATH), lib.version()))
say("# %d rounds x %d calls after %d warm-up calls; device events; every shape alternates with ntt_copy_probe of the same bytes" % (ROUNDS, CALLS, WARM))
automorphism()
key_product()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
