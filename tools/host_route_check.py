#!/usr/bin/env python3
"""tools/host_route_check.py ledger | bench: the host routes of csrc/host/host_transforms.inc, host_products.inc and host_ntt_domain.inc
(which launch record a call fills, with which values), one library against another.  NTT_LIB selects the library, as everywhere in
tools/ (tools/build_head.sh builds the parent commit's into build/libntt_prev.so).

  ledger   a fixed list of calls that reaches every branch of those routes at the smallest shape that does, on inputs from
           ntt_fill_uniform with fixed seeds, in ONE child process under `rocprofv3 --kernel-trace`.  Per call: its label, a digest of
           ntt_poly_checksum over every buffer of the call (outputs and the operands a route uses as scratch), and for every dispatch
           the kernel, grid, workgroup and LDS size from the trace.  Results are integers: the ledgers of two libraries that take the
           same routes are byte-identical (NTT_LIB=build/libntt_prev.so ... ledger > a; ... ledger > b; cmp a b).
  bench    the routes at sizes a user would run (1024 polynomials), the parent's library (--prev) against this tree's, on the method of
           tools/moddown_refactor_bench.py: device events, 3 warm-up calls per shape, windows of 10 calls, the two libraries in ALTERNATING child
           processes, a child's figure = the median of its windows; per size the warm-up is repeated until it covers 60 ms of device
           work.  Pass condition per shape: the tree's range overlaps the parent's, or the tree's slowest round is no further from the parent's median than the parent's own spread in this run.

50-bit primes for the FP64 policies, 59-bit primes for the integer ones (f64 / int = the wide integer policy / ref = the reference's
butterflies / r4 = the radix-4 formulation)."""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("ledger", "bench"))
ap.add_argument("--prev", default=os.path.join(ROOT, "build", "libntt_prev.so"), help="bench: the parent commit's library")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--quick", action="store_true", help="bench: fewer rounds, calls and polynomials (a smoke run of the tool)")
ap.add_argument("--child", nargs="?", const="0", help=argparse.SUPPRESS)
a = ap.parse_args()

POOL_WORDS = 1 << 23  # the largest operand of the ledger: 64 polynomials of 2^17 words


class Rig:
    """plans by (size, policy, options) and a pool of device buffers"""

    def __init__(self, nbufs, words):
        import ontt
        self.lib = lib = ontt.load()
        self.opt = {"one_pass": lib.OPT_ONE_PASS, "xcd_local": lib.OPT_XCD_LOCAL, "two_phase": lib.OPT_TWO_PHASE, "chunk_mib": lib.OPT_CHUNK_MIB,
                    "dot_fused": lib.OPT_DOT_FUSED, "fused_product": lib.OPT_FUSED_PRODUCT, "rns_launch": lib.OPT_RNS_LAUNCH}
        self.bufs = [lib.DeviceBuffer(words) for _ in range(nbufs)]
        self.words = words
        self.plans = {}

    def plan(self, logn, kind, skip=0, **opts):
        key = (logn, kind, skip, tuple(sorted(opts.items())))
        if key not in self.plans:
            lib, n = self.lib, 1 << logn
            q = lib.find_prime(50 if kind == "f64" else 59, n, skip)
            arith = {"f64": lib.ARITH_AUTO, "int": lib.ARITH_AUTO, "ref": lib.ARITH_U64, "r4": lib.ARITH_U64_R4}[kind]
            p = lib.Plan(n, q, lib.min_root(q, n), arith=arith)
            for k, v in opts.items():
                p.set_option(self.opt[k], v)
            self.plans[key] = p
        return self.plans[key]

    def table(self, base, count, stride_words):
        """a device table of `count` polynomial addresses stride_words apart, last polynomial first"""
        import numpy as np
        t = self.lib.DeviceBuffer(count)
        t.upload(np.array([base + 8 * stride_words * (count - 1 - i) for i in range(count)], dtype=np.uint64))
        return t


# ----------------------------------------------------------------------------------------------------------------------------
# ledger
# ----------------------------------------------------------------------------------------------------------------------------
CHUNKED = dict(one_pass=0, xcd_local=0, chunk_mib=1)  # 2^15, 9 polynomials: chunks of 4, 4, 1


def ledger_calls(rig):
    """(label, N, modulus of the inputs, words per buffer, buffers, fn(pointers)) for every call of the ledger"""
    lib = rig.lib
    LZ, BC, ACC = lib.MUL_LAZY_IN, lib.MUL_B_BROADCAST, lib.MUL_ACCUMULATE
    calls = []

    def add(label, ps, words, nb, fn):
        ps = ps if isinstance(ps, list) else [ps]
        assert words <= rig.words and words % ps[0].N == 0 and nb <= len(rig.bufs), label
        calls.append((label, ps[0].N, min(p.q for p in ps), words, nb, fn))  # (inputs below every modulus of the call)

    def name(op, logn, kind, batch, opts, extra=""):
        return "%s 2^%d %s batch=%d%s%s" % (op, logn, kind, batch, "".join(" %s=%d" % kv for kv in sorted(opts.items())), extra)

    # transforms
    shapes = [(6, k, 3, {}) for k in ("f64", "int")] + [(14, k, 3, {}) for k in ("f64", "int")]
    for logn, kind, batch, opts in shapes:
        for inv in (False, True):
            for wide, lazy in ((False, False), (False, True), (True, False)):
                p = rig.plan(logn, kind, **opts)
                f = p.inv if inv else p.fwd
                add(name("inv" if inv else "fwd", logn, kind, batch, opts, " wide=%d lazy=%d" % (wide, lazy)), p, batch << logn, 1,
                    lambda b, f=f, batch=batch, wide=wide, lazy=lazy: f(b[0], batch, wide=wide, lazy=lazy))
    shapes = [(15, "f64", 2, dict(one_pass=1)), (15, "f64", 64, dict(xcd_local=1)), (17, "f64", 64, dict(xcd_local=1)), (15, "int", 64, dict(xcd_local=1)),
              (16, "f64", 2, dict(two_phase=1)), (15, "f64", 9, CHUNKED), (15, "int", 9, CHUNKED), (15, "r4", 2, {})]
    for logn, kind, batch, opts in shapes:
        for inv in (False, True):
            p = rig.plan(logn, kind, **opts)
            f = p.inv if inv else p.fwd
            add(name("inv" if inv else "fwd", logn, kind, batch, opts), p, batch << logn, 1, lambda b, f=f, batch=batch: f(b[0], batch))

    # products of operands in the NTT domain
    routes = [(5, 3, {}), (10, 3, dict(dot_fused=0)), (6, 3, {}), (14, 3, {}), (15, 64, dict(xcd_local=1)), (15, 9, CHUNKED)]
    for kind in ("f64", "int"):
        for logn, batch, opts in routes + [(15, 2, dict(one_pass=1))]:
            p, w = rig.plan(logn, kind, **opts), batch << logn
            if opts.get("one_pass") != 1:
                for k in (1, 3):
                    for fl in (0, LZ, BC):
                        add(name("inv_dot", logn, kind, batch, opts, " k=%d flags=%d" % (k, fl)), p, w, 1 + 2 * k,
                            lambda b, p=p, k=k, fl=fl, batch=batch: p.inv_dot(b[0], b[1:1 + k], b[1 + k:1 + 2 * k], batch, fl))
                for fl in (0, LZ):
                    add(name("mul_transformed", logn, kind, batch, opts, " flags=%d" % fl), p, w, 3,
                        lambda b, p=p, fl=fl, batch=batch: p.mul_transformed(b[0], b[1], b[2], batch, fl))
            for fl in (0, LZ, BC, ACC, LZ | BC | ACC):
                add(name("fwd_mul", logn, kind, batch, opts, " flags=%d" % fl), p, w, 3,
                    lambda b, p=p, fl=fl, batch=batch: p.fwd_mul(b[0], b[1], b[2], batch, fl))

    # coefficient-domain products
    shapes = [(8, "f64", 3, {}), (14, "f64", 3, {}), (14, "f64", 3, dict(fused_product=2)), (15, "f64", 64, dict(xcd_local=1)), (15, "f64", 9, CHUNKED),
              (14, "int", 3, {}), (15, "int", 9, CHUNKED)]
    for logn, kind, batch, opts in shapes:
        p = rig.plan(logn, kind, **opts)
        add(name("negacyclic_mul", logn, kind, batch, opts), p, batch << logn, 3, lambda b, p=p, batch=batch: p.negacyclic_mul(b[0], b[1], b[2], batch))
    p = rig.plan(14, "f64")
    add("negacyclic_mul 2^14 f64 batch=3 squaring", p, 3 << 14, 2, lambda b, p=p: p.negacyclic_mul(b[0], b[1], b[1], 3))
    for kind in ("f64", "int"):
        for lazy in (False, True):
            p = rig.plan(10, kind)
            add("pointwise_mul 2^10 %s batch=3 lazy=%d" % (kind, lazy), p, 3 << 10, 3, lambda b, p=p, lazy=lazy: p.pointwise_mul(b[0], b[1], b[2], 3, lazy_in=lazy))

    # the RNS slab forms, three limbs
    for logn, kind, batch, opts in ((14, "f64", 3, {}), (15, "f64", 22, dict(xcd_local=1)), (14, "int", 3, {})):
        n = 1 << logn
        for rl in (0, 1):
            ps = [rig.plan(logn, kind, s, rns_launch=rl, **opts) for s in range(3)]
            for lay in (None, (n, 4 * n)):
                w = 3 * batch * n if lay is None else 4 * batch * n
                tag = " rns_launch=%d %s" % (rl, "limb-major" if lay is None else "poly-major")
                add(name("rns_negacyclic_mul", logn, kind, batch, opts, tag), ps, w, 3,
                    lambda b, ps=ps, batch=batch, lay=lay: lib.rns_negacyclic_mul(ps, b[0], b[1], b[2], batch, layout=lay))
                add(name("rns_mul_transformed", logn, kind, batch, opts, tag), ps, w, 3,
                    lambda b, ps=ps, batch=batch, lay=lay: lib.rns_mul_transformed(ps, b[0], b[1], b[2], batch, layout=lay))
                for fl in (0, BC):
                    add(name("rns_inv_dot", logn, kind, batch, opts, tag + " k=2 flags=%d" % fl), ps, w, 5,
                        lambda b, ps=ps, batch=batch, lay=lay, fl=fl: lib.rns_inv_dot(ps, b[0], b[1:3], b[3:5], batch, fl, layout=lay))
                for fl in (0, BC | ACC):
                    add(name("rns_fwd_mul", logn, kind, batch, opts, tag + " flags=%d" % fl), ps, w, 3,
                        lambda b, ps=ps, batch=batch, lay=lay, fl=fl: lib.rns_fwd_mul(ps, b[0], b[1], b[2], batch, fl, layout=lay))

    # pointer batches: every operand a device table, single plan and three limbs (a polynomial's limbs side by side)
    shapes = [(14, "f64", 5, {}), (15, "f64", 64, {}), (15, "f64", 4, dict(one_pass=1)), (15, "f64", 5, dict(xcd_local=0)), (15, "ref", 5, {}), (14, "int", 5, {})]
    for logn, kind, count, opts in shapes:
        n = 1 << logn
        for nl in (1, 3):
            ps = [rig.plan(logn, kind, s, **opts) for s in range(nl)]
            w, tag = nl * count * n, " limbs=%d" % nl

            def tabs(b, m, count=count, n=n, nl=nl):
                return [rig.table(x, count, nl * n) for x in b[:m]]

            if opts.get("one_pass") != 1:
                for fl in (0, BC):
                    def f(b, fl=fl, ps=ps, nl=nl, count=count, n=n, tabs=tabs):
                        t = tabs(b, 5)
                        bb = [b[3], b[4]] if fl & BC else [t[3].ptr, t[4].ptr]
                        if nl == 1: ps[0].inv_dot_dev_ptrs(t[0].ptr, [t[1].ptr, t[2].ptr], bb, count, fl)
                        else: lib.rns_inv_dot_dev_ptrs(ps, t[0].ptr, [t[1].ptr, t[2].ptr], bb, count, n, fl)
                        return t
                    add(name("inv_dot_dev_ptrs", logn, kind, count, opts, tag + " k=2 flags=%d" % fl), ps, w, 5, f)

                def g(b, ps=ps, nl=nl, count=count, n=n, tabs=tabs):
                    t = tabs(b, 3)
                    if nl == 1: ps[0].negacyclic_mul_dev_ptrs(t[0].ptr, t[1].ptr, t[2].ptr, count)
                    else: lib.rns_negacyclic_mul_dev_ptrs(ps, t[0].ptr, t[1].ptr, t[2].ptr, count, n)
                    return t
                add(name("negacyclic_mul_dev_ptrs", logn, kind, count, opts, tag), ps, w, 3, g)
            for fl in (0, BC | ACC):
                def h(b, fl=fl, ps=ps, nl=nl, count=count, n=n, tabs=tabs):
                    t = tabs(b, 3)
                    bb = b[2] if fl & BC else t[2].ptr
                    if nl == 1: ps[0].fwd_mul_dev_ptrs(t[0].ptr, t[1].ptr, bb, count, fl)
                    else: lib.rns_fwd_mul_dev_ptrs(ps, t[0].ptr, t[1].ptr, bb, count, n, fl)
                    return t
                add(name("fwd_mul_dev_ptrs", logn, kind, count, opts, tag + " flags=%d" % fl), ps, w, 3, h)
    return calls


def ledger_child():
    """every call: buffers filled (ntt_fill_uniform, seeds by call and buffer), the call, the checksums -- 'CALL label' / 'SUMS digest'"""
    import numpy as np
    rig = Rig(7, POOL_WORDS)
    lib = rig.lib
    sums = lib.DeviceBuffer(POOL_WORDS >> 5)
    for idx, (label, n, q, words, nb, fn) in enumerate(ledger_calls(rig)):
        ptrs = [b.ptr for b in rig.bufs[:nb]]
        for j, ptr in enumerate(ptrs):
            lib.fill_uniform(ptr, words, q, 1000 * idx + j)
        keep = fn(ptrs)  # (device tables of a pointer batch stay alive until the call has run)
        h = hashlib.sha256()
        for ptr in ptrs:
            lib.poly_checksum(sums.ptr, ptr, n, words // n)
            h.update(np.ascontiguousarray(sums.download(words // n)).tobytes())
        del keep
        print("CALL %s\nSUMS %s" % (label, h.hexdigest()[:32]))
        sys.stdout.flush()


def kernel_name(s):
    """the kernel of a trace row without its parameter list and the code-object suffix"""
    s = re.sub(r"\.kd$", "", s.strip())
    depth = 0
    for i, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def ledger():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "ledger", "--child"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # (nothing is started after a child that ends uncleanly)
            raise SystemExit("the ledger's child ended with status %d:\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                rows += list(csv.DictReader(fh))
    rows.sort(key=lambda x: (int(x["Start_Timestamp"]), int(x.get("Dispatch_Id", 0))))

    def dims(row, what):
        keys = sorted(k for k in row if k.startswith(what))
        return "x".join(row[k] for k in keys)

    # a call's dispatches: after its fills, before its checksums
    groups, filling = [], False
    for row in rows:
        k = kernel_name(row["Kernel_Name"])
        if "fill_uniform_kernel" in k:
            if not filling: groups.append([])
            filling = True
        elif "checksum_kernel" in k:
            filling = False
        elif groups and not k.startswith("__amd_rocclr"):  # (the runtime's own copy kernels: table uploads, checksum downloads)
            filling = False
            lds = row.get("LDS_Block_Size", row.get("Group_Segment_Size", "?"))
            groups[-1].append("  %s grid %s wg %s lds %s" % (k, dims(row, "Grid_Size"), dims(row, "Workgroup_Size"), lds))
    lines = [l for l in r.stdout.splitlines() if l.startswith(("CALL ", "SUMS "))]
    labels = lines[0::2]
    if len(labels) != len(groups):
        raise SystemExit("%d calls, but the trace holds the dispatches of %d" % (len(labels), len(groups)))
    for i, g in enumerate(groups):
        print(lines[2 * i] + "\n" + lines[2 * i + 1])
        print("\n".join(g) if g else "  (no dispatch)")


# ----------------------------------------------------------------------------------------------------------------------------
# bench
# ----------------------------------------------------------------------------------------------------------------------------
def bench_child(rnd, quick):
    polys, calls, warm, windows = (128, 3, 2, 2) if quick else (1024, 10, 3, 3)
    rig = Rig(7, polys << 17)
    lib = rig.lib
    e0, e1 = lib.Event(), lib.Event()
    out = {}
    for logn in (14, 15, 16, 17):
        n, fns = 1 << logn, {}
        b = [x.ptr for x in rig.bufs]
        for x in b:
            lib.fill_uniform(x, polys * n, lib.find_prime(50, n, 0), 7)
        for xcd in ((-1,) if logn == 14 else (1, 0)):
            p = rig.plan(logn, "f64", **({} if xcd < 0 else dict(xcd_local=xcd)))
            tag = "2^%d %s" % (logn, {-1: "one launch", 1: "one-launch form", 0: "per chunk"}[xcd])
            fns["fwd " + tag] = lambda p=p: p.fwd(b[0], polys)
            fns["inv_dot k=1 " + tag] = lambda p=p: p.inv_dot(b[0], b[1:2], b[2:3], polys)
            fns["inv_dot k=3 " + tag] = lambda p=p: p.inv_dot(b[0], b[1:4], b[4:7], polys)
            fns["fwd_mul " + tag] = lambda p=p: p.fwd_mul(b[0], b[1], b[2], polys)
            fns["negacyclic_mul " + tag] = lambda p=p: p.negacyclic_mul(b[0], b[1], b[2], polys)
        if logn == 16:
            p, t = rig.plan(logn, "f64"), [rig.table(x, polys, n) for x in b[:3]]
            fns["inv_dot_dev_ptrs k=1 2^16"] = lambda p=p, t=t: p.inv_dot_dev_ptrs(t[0].ptr, [t[1].ptr], [t[2].ptr], polys)
            fns["fwd_mul_dev_ptrs 2^16"] = lambda p=p, t=t: p.fwd_mul_dev_ptrs(t[0].ptr, t[1].ptr, t[2].ptr, polys)
            fns["negacyclic_mul_dev_ptrs 2^16"] = lambda p=p, t=t: p.negacyclic_mul_dev_ptrs(t[0].ptr, t[1].ptr, t[2].ptr, polys)
        names = sorted(fns)
        names = names[rnd % len(names):] + names[:rnd % len(names)]
        # warm-up: `warm` calls of every shape, repeated until 60 ms of device work have passed -- whatever is measured first after an idle
        # gap (plan creation, fills) reads low while the clocks settle (profiles/r05/clock_settling_after_idle.txt, bench_warmup_length.txt);
        # the 2^14 shapes take 0.06 .. 0.2 ms a call, so three calls each leave them inside that window
        warmed = 0.0
        while warmed < 60.0:
            e0.record()
            for name in names:
                for _ in range(warm):
                    fns[name]()
            e1.record()
            lib.stream_sync()
            warmed += e1.elapsed_ms_since(e0)
        t = {name: [] for name in names}
        for _ in range(windows):
            for name in names:
                e0.record()
                for _ in range(calls):
                    fns[name]()
                e1.record()
                lib.stream_sync()
                t[name].append(e1.elapsed_ms_since(e0) / calls)
        for name in names:
            out[name] = statistics.median(t[name])
    print(json.dumps(out))


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def bench():
    cur = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "libntt_mi355x.so")
    rounds_n = 2 if a.quick else a.rounds
    print("# tools/host_route_check.py bench")
    print("# tree library   sha256 %s" % sha(cur))
    print("# parent library sha256 %s (%s)" % (sha(a.prev), os.path.relpath(a.prev, ROOT)))
    print("# %d rounds of alternating child processes (parent, tree, ...); %d polynomials, FP64 policy; ms per call, min..max over the rounds"
          % (rounds_n, 128 if a.quick else 1024))
    rounds = {"prev": [], "cur": []}
    for rnd in range(rounds_n):
        for which in ("prev", "cur"):
            env = dict(os.environ)
            if which == "prev": env["NTT_LIB"] = a.prev
            else: env.pop("NTT_LIB", None)
            args = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "bench", "--child", str(rnd)] + (["--quick"] if a.quick else [])
            r = subprocess.run(args, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # (nothing is started after a child that ends uncleanly)
                raise SystemExit("child %s of round %d ended with status %d: %s" % (which, rnd, r.returncode, r.stderr[-2000:]))
            rounds[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    outside, ratios = 0, []
    for k in sorted(rounds["prev"][0], key=lambda s: (s.split("2^")[1][:2], s)):
        p, t = [r[k] for r in rounds["prev"]], [r[k] for r in rounds["cur"]]
        pm, tm = statistics.median(p), statistics.median(t)
        overlap = min(t) <= max(p) and min(p) <= max(t)
        near = max(t) - pm <= max(p) - min(p)
        verdict = "pass (ranges overlap)" if overlap else "pass (within the parent's spread)" if near else "OUTSIDE"
        outside += verdict == "OUTSIDE"
        ratios.append(tm / pm)
        print("%-40s parent %8.4f..%8.4f (median %8.4f)  tree %8.4f..%8.4f (median %8.4f)  tree/parent median %.3f  %s"
              % (k, min(p), max(p), pm, min(t), max(t), tm, tm / pm, verdict))
        sys.stdout.flush()
    print("# %d shapes, %d outside the pass condition; tree / parent medians %.3f .. %.3f" % (len(ratios), outside, min(ratios), max(ratios)))
    sys.exit(1 if outside else 0)


if a.mode == "ledger":
    ledger_child() if a.child is not None else ledger()
else:
    bench_child(int(a.child), a.quick) if a.child is not None else bench()
