"""Recipe table: for every shipped kernel instance (tests/kernel_inventory.py) the call that launches it, checked word for word
against the oracle.

One function per family maps the instance's template arguments to a concrete call: entry point, modulus (the largest
NTT-friendly prime that puts the plan in the instance's policy and headroom class), plan options, batch (ragged, on the
launching side of every threshold the dispatch code names) and direction.  A function returns None for arguments no call
can reach; such instances belong in ALLOWLIST with the dispatch line that rules them out.

Instances no recipe covers yet are pinned in tests/golden/uncovered_kernel_instances.txt (UNCOVERED_LIST):
tests/test_kernel_inventory.py fails on any shipped instance that is neither claimed, allowlisted nor pinned there.

Beside the canonical case every single-limb transform instance that carries the run-time wide-input and lazy-output paths
gets a WIDE case (inputs anywhere in [0,8q), 8q-1 among them) and a LAZY case (outputs checked modulo q and inside the lazy
range).  team_kernel has no such cases: team_applies (host_transforms.inc) sends wide and lazy calls to the per-pass launches.

Run as a script (the launch proof of tests/test_gpu_kernel_instances.py runs it under a kernel trace):
    python3 tests/kernel_recipes.py [substring ...]     every case whose id contains one of the substrings (default: all)
    python3 tests/kernel_recipes.py --precedence transform|fwd_mul     the route-precedence call (precedence_probe)
"""
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kernel_inventory  # noqa: E402

# instances no recipe covers yet, one normalised key per line: the issue's remaining families (fused_kernel, the product, dot
# and mul kernels, the pointwise kernels, the plain host kernels).  Pinned so that a new instantiation in any family fails
# tests/test_kernel_inventory.py until a recipe claims it, and so that the list can only shrink as recipes land.
UNCOVERED_LIST = os.path.join(ROOT, "tests", "golden", "uncovered_kernel_instances.txt")


def uncovered():
    with open(UNCOVERED_LIST) as f:
        return {line.strip() for line in f if line.strip() and not line.startswith("#")}


# key -> reason (the dispatch line that rules the instance out)
ALLOWLIST = {}

Case = collections.namedtuple("Case", "id inst run")

# --------------------------------------------------------------------------------------------------------------------
# moduli: the largest prime of each policy / headroom class (found once per (N, policy), by the plan's own classification)
# --------------------------------------------------------------------------------------------------------------------
_prime_cache = {}


def _classify(lib, n, q, arith):
    try:
        p = lib.Plan(n, q, lib.min_root(q, n), arith=arith)
    except lib.NttError:  # (a modulus the policy refuses: the search goes on below it)
        return None
    info = p.info()
    p.destroy()
    return info["arith"], info["f64_class"]


def policy_plan_args(lib, policy, ksh, n):
    """(arith, q, want_info) for the instance's policy: arith to pass to Plan, and the (arith, f64_class) info the plan must
    report (ntt_plan_info: 52 = ArithF64W, 100 + K = ArithU64X<K>)"""
    if policy == "ArithF64":
        return lib.ARITH_AUTO, range(52, 20, -1), (lib.ARITH_F64, ksh)
    if policy == "ArithF64W":
        return lib.ARITH_AUTO, range(52, 45, -1), (lib.ARITH_F64, 52)
    if policy.startswith("ArithU64X<"):
        k = int(policy[len("ArithU64X<"):-1])
        return lib.ARITH_AUTO, range(61, 52, -1), (lib.ARITH_U64, 100 + k)
    if policy == "ArithU64":
        return lib.ARITH_U64, range(61, 52, -1), (lib.ARITH_U64, 0)
    if policy == "ArithU64R4":
        return lib.ARITH_U64_R4, range(60, 52, -1), (lib.ARITH_U64_R4, 0)
    raise ValueError(policy)


def prime_for(lib, policy, ksh, n, skip=0):
    """the largest prime q = 1 mod 2N (skip: the next ones below it) whose plan lands in (policy, class)"""
    key = (policy, ksh, n, skip)
    if key not in _prime_cache:
        arith, bits_range, want = policy_plan_args(lib, policy, ksh, n)
        found = None
        for bits in bits_range:
            q = lib.find_prime(bits, n, skip)
            got = _classify(lib, n, q, arith)
            if got == want:
                found = q
                break
        assert found, "no prime for %s class %s at N=%d" % (policy, ksh, n)
        _prime_cache[key] = found
    return _prime_cache[key]


def make_plans(lib, oracle, policy, ksh, n, nlimbs):
    arith = policy_plan_args(lib, policy, ksh, n)[0]
    out = []
    for skip in range(nlimbs):
        q = prime_for(lib, policy, ksh, n, skip)
        w = lib.min_root(q, n)
        out.append((lib.Plan(n, q, w, arith=arith), q, oracle.ctx(n, q, w)))
    return out


def inputs(oracle, n, q, batch, seed):
    """uniform canonical words, the extremes of the canonical range in the first words of the first polynomial"""
    a = oracle.fill_uniform(batch * n, q, seed)
    ext = [0, 1, q - 1, q // 2, q // 2 + 1]
    a[:len(ext)] = np.array(ext, dtype=np.uint64)
    return a


# --------------------------------------------------------------------------------------------------------------------
# transforms: one slab (single limb) or an RNS set [limb][batch][N] in one launch over the limbs
# --------------------------------------------------------------------------------------------------------------------
def _wide(oracle, a, q, seed):
    """the same residues as a, lifted anywhere into [0,8q); the canonical extremes of the first words lifted to the top
    (7q, 7q+1, 8q-1, ...)"""
    k = oracle.fill_uniform(a.size, 8, seed)
    w = a + np.uint64(q) * k
    w[:5] = a[:5] + np.uint64(7 * q)
    return w


def _transform_case(inst, policy, ksh, m, inverse, batch, nlimbs, options, mode=""):
    """mode "": canonical inputs and outputs; "wide": inputs in [0,8q) (ntt_*_batch_wide); "lazy": lazy outputs
    (ntt_*_batch_lazy: forward [0,4q) -- radix-4 policy [0,8q) --, inverse [0,2q))"""
    n = 1 << m

    def run(lib, oracle):
        ps = make_plans(lib, oracle, policy, ksh, n, nlimbs)
        try:
            for p, _, _ in ps:
                for o, v in options:
                    p.set_option(getattr(lib, o), v)
            a = np.concatenate([inputs(oracle, n, q, batch, 0x1357 + 17 * i) for i, (_, q, _) in enumerate(ps)])
            x = _wide(oracle, a, ps[0][1], 0x77) if mode == "wide" else a
            buf = lib.DeviceBuffer(x.size).upload(x)
            try:
                if nlimbs == 1:
                    (ps[0][0].inv if inverse else ps[0][0].fwd)(buf.ptr, batch, wide=mode == "wide", lazy=mode == "lazy")
                else:
                    lib.set_rns_launch([p for p, _, _ in ps], 0)
                    (lib.rns_inv if inverse else lib.rns_fwd)([p for p, _, _ in ps], buf.ptr, batch)
                got = buf.download()
            finally:
                buf.free()
            for i, (_, q, cx) in enumerate(ps):
                lo, hi = i * batch * n, (i + 1) * batch * n
                want = cx.inv(a[lo:hi]) if inverse else cx.fwd(a[lo:hi])
                g = got[lo:hi]
                if mode == "lazy":
                    bound = 2 * q if inverse else (8 * q if policy == "ArithU64R4" else 4 * q)
                    assert int(g.max()) < bound, "%s: lazy output %#x outside [0,%#x)" % (kernel_inventory.case_id(inst), int(g.max()), bound)
                    g = g % np.uint64(q)
                bad = np.nonzero(g != want)[0]
                assert bad.size == 0, "%s%s: limb %d q=%#x: %d words differ, first at polynomial %d word %d" % (
                    kernel_inventory.case_id(inst), mode and "-" + mode, i, q, bad.size, bad[0] // n, bad[0] % n)
        finally:
            for p, _, _ in ps:
                p.destroy()
    return Case(kernel_inventory.case_id(inst) + (mode and "-" + mode), inst, run)


def _with_wide_and_lazy(inst, policy, ksh, m, inverse, batch, nlimbs, options):
    """the canonical case; single-limb calls also the wide-input and the lazy-output case of the same launch"""
    modes = ("",) if nlimbs > 1 else ("", "wide", "lazy")
    return [_transform_case(inst, policy, ksh, m, inverse, batch, nlimbs, options, mode) for mode in modes]


def _nlimbs(multi):
    return 2 if multi else 1


def recipe_onepass(inst):
    """onepass_kernel<A, INV, KSH, MULTI>: N = 2^15, NTT_OPT_ONE_PASS 1 (host_transforms.inc, run_transform)"""
    a = inst.args
    return _with_wide_and_lazy(inst, inst.policy, a["KSH"], 15, a["INV"], 5 if not a["MULTI"] else 3, _nlimbs(a["MULTI"]),
                               (("OPT_ONE_PASS", 1),))


def recipe_twophase(inst):
    """twophase_kernel<A, LEAD, INV, KSH>: N = 2^(14 + LEAD), NTT_OPT_TWO_PHASE 1, the XCD-local launch off"""
    a = inst.args
    return _with_wide_and_lazy(inst, inst.policy, a["KSH"], 14 + a["LEAD"], a["INV"], 3, 1,
                               (("OPT_TWO_PHASE", 1), ("OPT_XCD_LOCAL", 0)))


def recipe_team(inst):
    """team_kernel<A, LEAD, INV, KSH, MULTI>: N = 2^(12 + LEAD), NTT_OPT_XCD_LOCAL 1, from 64 polynomials x limbs on
    (host_transforms.inc, team_applies); 2^15 with FP64: the explicit option wins over the automatic one-pass choice.
    Canonical words only: wide and lazy calls take the per-pass launches (team_applies)."""
    a = inst.args
    multi = a["MULTI"]
    return [_transform_case(inst, inst.policy, a["KSH"], 12 + a["LEAD"], a["INV"], 33 if multi else 65, _nlimbs(multi),
                            (("OPT_XCD_LOCAL", 1),))]


def recipe_column(inst):
    """column_kernel<A, R, INV, KSH, MULTI>: the leading stages of N > 2^14 (ntt_passplan.h, make_passes): R stages ahead of
    2^14-point blocks (N = 2^(14 + R), R = 1, 2) or of 2^12-point blocks (N = 2^(12 + R), R = 3, 4), NTT_OPT_BLOCK_LOG
    fixing the block; the one-pass, two-phase and XCD-local launches off.  ArithU64R4 (make_passes_r4): one radix-4 level
    ahead of the blocks at 2^15, two at 2^17.  The forward wide case runs the column pass's fold of [0,8q) inputs (the
    first pass of the transform); the inverse lazy case its lazy output (the last pass)."""
    a = inst.args
    r, multi = a["R"], a["MULTI"]
    if inst.policy == "ArithU64R4":
        if r not in (2, 4) or multi:
            return None
        return _with_wide_and_lazy(inst, inst.policy, a["KSH"], 15 if r == 2 else 17, a["INV"], 3, 1, ())
    m, blog = (14 + r, 14) if r <= 2 else (12 + r, 12)
    opts = (("OPT_BLOCK_LOG", blog), ("OPT_XCD_LOCAL", 0))
    if inst.policy in ("ArithF64", "ArithF64W"):
        opts += (("OPT_ONE_PASS", 0), ("OPT_TWO_PHASE", 0))
    return _with_wide_and_lazy(inst, inst.policy, a["KSH"], m, a["INV"], 3, _nlimbs(multi), opts)


RECIPES = {
    "onepass_kernel": recipe_onepass,
    "twophase_kernel": recipe_twophase,
    "team_kernel": recipe_team,
    "column_kernel": recipe_column,
}


def claims(inst):
    """the recipes that claim the instance (a list: the inventory test wants exactly one)"""
    return [fam for fam, fn in RECIPES.items() if fam == inst.family and fn(inst)]


def cases(inst_map=None):
    inst_map = inst_map or kernel_inventory.instances()
    out = []
    for key in sorted(inst_map):
        inst = inst_map[key]
        fn = RECIPES.get(inst.family)
        if fn is None or key in ALLOWLIST:
            continue
        out += fn(inst) or []
    return out


def covered_keys(inst_map=None):
    return {c.inst.key for c in cases(inst_map)}


def precedence_probe(lib, oracle, route):
    """one call at N = 2^15 with a 50-bit prime, NTT_OPT_XCD_LOCAL 1, 131 polynomials: the transform (route "transform": fwd
    and inv) or the NTT-domain product (route "fwd_mul"), checked against the oracle.  The explicit option must win over the
    automatic one-pass choice (a kernel trace of this call shows team_kernel / team_mul_kernel, no one-pass kernel)."""
    n, batch = 1 << 15, 131
    q = lib.find_prime(50, n)
    w = lib.min_root(q, n)
    cx, plan = oracle.ctx(n, q, w), lib.Plan(n, q, w)
    plan.set_option(lib.OPT_XCD_LOCAL, 1)
    a = inputs(oracle, n, q, batch, 0xC0DE)
    da = lib.DeviceBuffer(a.size).upload(a)
    if route == "transform":
        plan.fwd(da.ptr, batch)
        f = da.download()
        assert np.array_equal(f, cx.fwd(a)), "forward transform differs from the oracle"
        plan.inv(da.ptr, batch)
        assert np.array_equal(da.download(), a), "inverse transform does not round-trip"
    else:
        bh = cx.fwd(inputs(oracle, n, q, batch, 0xB0B))
        db, dc = lib.DeviceBuffer(a.size).upload(bh), lib.DeviceBuffer(a.size)
        plan.fwd_mul(dc.ptr, da.ptr, db.ptr, batch)
        assert np.array_equal(dc.download(), oracle.pointwise(cx.fwd(a), bh, q)), "fwd(a) * b^ differs from the oracle"
        db.free(), dc.free()
    da.free()
    plan.destroy()


def main(argv):
    import ontt
    from oracle_binding import Oracle
    lib, oracle = ontt.load(), Oracle()
    if argv and argv[0] == "--precedence":
        precedence_probe(lib, oracle, argv[1])
        print("precedence probe ok:", argv[1], flush=True)
        return 0
    sel = [c for c in cases() if not argv or any(s in c.id for s in argv)]
    t0, failed = time.time(), []
    for c in sel:
        try:
            c.run(lib, oracle)
        except AssertionError as e:
            failed.append((c.id, str(e)))
            print("FAIL", c.id, e, flush=True)
    print("ran %d cases in %.1f s, %d failed" % (len(sel), time.time() - t0, len(failed)), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
