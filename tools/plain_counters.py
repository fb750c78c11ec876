#!/usr/bin/env python3
"""tools/plain_counters.py: ntt_rns_to_plain_batch (both modes) at 2^14 x 1024 polynomials, L = 1, 4, 16 limbs of 50-bit primes, t = 65537,
three calls each, and ntt_copy_probe at the same bytes -- the workload of a counter pass:
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \\
      --output-format csv -d DIR -- python3 tools/plain_counters.py
(counters on their own: nothing traced in the same run).  With --summarise DIR it prints, per kernel and grid, the counters' means and
the shares of the wave cycles spent parked (SQ_WAIT_ANY), stalled at issue (SQ_WAIT_INST_ANY) and issuing (SQ_ACTIVE_INST_ANY)."""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import ontt
    lib = ontt.load()
    n, batch, t = 1 << 14, 1024, 65537
    qs = [lib.find_prime(50, n, k) for k in range(16)]
    plans = [lib.Plan(n, q, lib.min_root(q, n)) for q in qs]
    per = batch * n
    src, dst, probe = lib.DeviceBuffer(16 * per), lib.DeviceBuffer(per), lib.DeviceBuffer(17 * per // 2)
    for l, q in enumerate(qs):
        lib.fill_uniform(src.ptr + 8 * l * per, per, q, 77 + l)
    for nl in (1, 4, 16):
        for flags in (0, lib.PLAIN_SCALE):
            for _ in range(3):
                lib.rns_to_plain(plans[:nl], dst.ptr, src.ptr, t, batch, flags)
        for _ in range(3):
            lib.copy_probe(probe.ptr, src.ptr, per * (nl + 1) // 2)
    dst.download(8)


def summarise(d):
    rows = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if "plain_kernel" not in k and "copy" not in k:
                continue
            rows[(k.split("(")[0].replace("void ", "").replace("ntt::", "")[:28], r["Dispatch_Id"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for (k, disp), c in sorted(rows.items(), key=lambda kv: int(kv[0][1])):
        v = {name: sum(x) for name, x in c.items()}
        wc = v.get("SQ_WAVE_CYCLES", 0) or 1
        print("%-28s dispatch %-3s  wave cycles %.3e  parked %.2f  issue-stalled %.2f  issuing %.2f  (VALU %.2f)  VALU insts %.3e  GUI_ACTIVE %.3e" % (
            k, disp, wc, v.get("SQ_WAIT_ANY", 0) / wc, v.get("SQ_WAIT_INST_ANY", 0) / wc, v.get("SQ_ACTIVE_INST_ANY", 0) / wc,
            v.get("SQ_ACTIVE_INST_VALU", 0) / wc, v.get("SQ_INSTS_VALU", 0), v.get("GRBM_GUI_ACTIVE", 0)))


if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2])
else:
    run()
