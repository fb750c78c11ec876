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

The product families (fused_product_kernel, fused_product_small_kernel, team_product_kernel) are driven through
ntt_negacyclic_mul_batch (both operands as coefficients: BOTH / FOUR), ntt_mul_transformed_batch (one operand given transformed,
once with canonical and once with the highest lazy words the header admits), their RNS twins on a padded limb-major layout
(MULTI) and the device-pointer-table entry points over shuffled, irregularly spaced records (PTRS).  NTT_OPT_MAX_GRID shrinks
the grids of the persistent block kernels so that the smallest batch already runs every path of their loops: some workgroups
wrap twice and others once in the same launch (next block prefetched / last block), the small-size kernels end on a partly
dead group of sub-blocks.  Every word of every polynomial of every limb is compared with inv(fwd(a) (.) fwd(b)) of the oracle;
operands the header promises to leave alone, the padding between polynomials and limbs and a sentinel polynomial behind the
output must come back unchanged.  The pointwise kernels (pointwise_kernel, pointwise_acc_kernel, pointwise_ptrs_kernel) get one
case per instance through the entry point that reaches it, with 4q-1 x 4q-1 among the lazy operands and q-1 + q-1 in the
accumulating forms.

Run as a script (the launch proof of tests/test_gpu_kernel_instances.py runs it under a kernel trace, one family per child):
    python3 tests/kernel_recipes.py [substring ...]     every case whose id contains one of the substrings (default: all)
    python3 tests/kernel_recipes.py --family NAME       every case of exactly that kernel family
    (--times beside either: the wall time of every case)
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

# instances no recipe covers yet, one normalised key per line: the remaining families (fused_kernel, the dot and mul kernels,
# the plain host kernels).  Pinned so that a new instantiation in any family fails
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


# --------------------------------------------------------------------------------------------------------------------
# products c = a * b in Z_q[X]/(X^N+1): slabs (one limb dense, an RNS set on a padded limb-major layout) or pointer tables
# --------------------------------------------------------------------------------------------------------------------
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)

_ref_cache = collections.OrderedDict()


def _readonly(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def _lazy_limit(q):
    """one past the highest lazy word ntt_mul_transformed_batch admits (include/ntt_mi355x.h, NTT_MUL_LAZY_IN): anywhere in
    [0,4q) and below 2^53"""
    return min(4 * q, 1 << 53)


def _product_reference(oracle, cx, n, q, batch, limb, given):
    """(a, b, want) of one limb, computed once and shared (read-only) by the cases on the same operands: a, b from inputs(), the
    last polynomial of both q-1 in every word; given: b is replaced by b^ = fwd(b) -- canonical words, among the first ones 0,
    q-1 and the residue of the highest admissible lazy word --; want = inv(fwd(a) (.) b^)"""
    key = (n, q, batch, limb, given)
    if key in _ref_cache:
        _ref_cache.move_to_end(key)
        return _ref_cache[key]
    a = inputs(oracle, n, q, batch, 0x2468 + 17 * limb)
    b = inputs(oracle, n, q, batch, 0xB0B + 29 * limb)
    a[-n:] = np.uint64(q - 1)
    b[-n:] = np.uint64(q - 1)
    bh = cx.fwd(b)
    if given:
        bh[:3] = np.array([0, q - 1, (_lazy_limit(q) - 1) % q], dtype=np.uint64)
        b = bh
    want = cx.inv(oracle.pointwise(cx.fwd(a), bh, q))
    assert int(want.max()) < q
    _ref_cache[key] = _readonly(a, b, want)
    while len(_ref_cache) > 4:
        _ref_cache.popitem(last=False)
    return _ref_cache[key]


def _lift_lazy(oracle, bh, q, seed):
    """the residues of bh as lazy words anywhere below _lazy_limit(q); the first three as high as they go: the largest multiple
    of q, the largest word = q-1 mod q, and the highest admissible word itself"""
    kmax = (np.uint64(_lazy_limit(q) - 1) - bh) // np.uint64(q)
    k = np.minimum(oracle.fill_uniform(bh.size, 4, seed), kmax)
    k[:3] = kmax[:3]
    w = bh + k * np.uint64(q)
    assert int(w[2]) == _lazy_limit(q) - 1 and int(w.max()) < _lazy_limit(q)
    return w


def _slab_layout(n, nlimbs, batch):
    """(limb stride, polynomial stride, words with a sentinel polynomial behind the last one): one limb dense (the single-plan
    entry points take [batch][N]); an RNS set limb-major with padding behind every polynomial and every limb, so that a kernel
    that assumes dense limbs or polynomials reads and writes the wrong words"""
    if nlimbs == 1:
        return batch * n, n, batch * n + n
    ps = n + 32
    ls = batch * ps + 256
    return ls, ps, nlimbs * ls + n


def _slab_image(per_limb, n, batch, layout):
    ls, ps, total = layout
    img = np.full(total, GUARD, dtype=np.uint64)
    for l, x in enumerate(per_limb):
        img[l * ls:l * ls + batch * ps].reshape(batch, ps)[:, :n] = x.reshape(batch, n)
    return img


def _slab_polys(img, n, nlimbs, batch, layout):
    ls, ps, _ = layout
    return [img[l * ls:l * ls + batch * ps].reshape(batch, ps)[:, :n].reshape(-1) for l in range(nlimbs)]


def _assert_words(cid, what, got, want, n, limb, q):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %s: limb %d q=%#x: %d words differ, first at polynomial %d word %d (got %#x, want %#x)" % (
        cid, what, limb, q, bad.size, bad[0] // n, bad[0] % n, int(got[bad[0]]), int(want[bad[0]]))


def _assert_unwritten(cid, what, got, before, n, nlimbs, batch, layout):
    """every word outside the polynomials (padding between polynomials and limbs, the sentinel polynomial behind the last one)
    is what it was"""
    pad = np.ones(got.size, dtype=bool)
    ls, ps, _ = layout
    for l in range(nlimbs):
        pad[l * ls:l * ls + batch * ps].reshape(batch, ps)[:, :n] = False
    bad = np.nonzero(pad & (got != before))[0]
    assert bad.size == 0, "%s: %s: %d words outside the polynomials were written, first at word %d of the buffer" % (
        cid, what, bad.size, bad[0])


def _run_slab(lib, cid, plans, qs, n, batch, entry, flags, a, b, want, a_kept, b_kept):
    nl = len(plans)
    lay = _slab_layout(n, nl, batch)
    ia, ib = _slab_image(a, n, batch, lay), _slab_image(b, n, batch, lay)
    ic = np.full(lay[2], GUARD, dtype=np.uint64)
    da, db, dc = (lib.DeviceBuffer(lay[2]).upload(x) for x in (ia, ib, ic))
    try:
        if nl == 1 and entry == "mul":
            plans[0].negacyclic_mul(dc.ptr, da.ptr, db.ptr, batch)
        elif nl == 1:
            plans[0].mul_transformed(dc.ptr, da.ptr, db.ptr, batch, flags)
        elif entry == "mul":
            lib.rns_negacyclic_mul(plans, dc.ptr, da.ptr, db.ptr, batch, layout=lay[:2])
        else:
            lib.rns_mul_transformed(plans, dc.ptr, da.ptr, db.ptr, batch, flags, layout=lay[:2])
        ga, gb, gc = da.download(), db.download(), dc.download()
    finally:
        da.free(), db.free(), dc.free()
    for l, g in enumerate(_slab_polys(gc, n, nl, batch, lay)):
        _assert_words(cid, "c", g, want[l], n, l, qs[l])
    _assert_unwritten(cid, "c", gc, ic, n, nl, batch, lay)
    for what, kept, g, before in (("a", a_kept, ga, ia), ("b", b_kept, gb, ib)):
        if kept:
            assert np.array_equal(g, before), "%s: operand %s was written (the header leaves it as it was)" % (cid, what)
        else:
            _assert_unwritten(cid, what, g, before, n, nl, batch, lay)


def _run_tables(lib, cid, plans, qs, n, count, a, b, want, kept):
    """the three operands as device tables of `count` pointers into one pool: every polynomial (RNS: its limbs, n + 16 words
    apart behind the entry) at a place of its own, the operands interleaved, shuffled, no two gaps alike -- a kernel that
    computes slab offsets instead of reading the tables produces wrong words"""
    nl = len(plans)
    lstride = n + 16
    rec = (nl - 1) * lstride + n
    rng = np.random.default_rng(0x7AB1E + n + count)
    gaps = rng.integers(1, 40, size=3 * count) + np.arange(3 * count) % 7
    starts = np.cumsum(gaps + rec) - rec
    words = int(starts[-1] + rec + n)
    offs = starts[rng.permutation(3 * count)].reshape(3, count)
    img = np.full(words, GUARD, dtype=np.uint64)
    for o, src in ((0, a), (1, b)):
        for l in range(nl):
            for p in range(count):
                at = int(offs[o][p]) + l * lstride
                img[at:at + n] = src[l][p * n:(p + 1) * n]
    pool = lib.DeviceBuffer(words).upload(img)
    tabs = [lib.DeviceBuffer(count).upload((np.uint64(pool.ptr) + np.uint64(8) * offs[o].astype(np.uint64))) for o in range(3)]
    try:
        if nl == 1:
            plans[0].negacyclic_mul_dev_ptrs(tabs[2].ptr, tabs[0].ptr, tabs[1].ptr, count)
        else:
            lib.rns_negacyclic_mul_dev_ptrs(plans, tabs[2].ptr, tabs[0].ptr, tabs[1].ptr, count, lstride)
        got = pool.download()
    finally:
        pool.free()
        for t in tabs:
            t.free()
    written = np.zeros(words, dtype=bool)
    for l in range(nl):
        g = np.concatenate([got[int(offs[2][p]) + l * lstride:int(offs[2][p]) + l * lstride + n] for p in range(count)])
        _assert_words(cid, "c", g, want[l], n, l, qs[l])
        for o in ((2,) if kept else (0, 1, 2)):   # (above 2^14 a and b are scratch: only what lies between the polynomials stays)
            for p in range(count):
                at = int(offs[o][p]) + l * lstride
                written[at:at + n] = True
    bad = np.nonzero(~written & (got != img))[0]
    assert bad.size == 0, "%s: %d words outside %s were written, first at word %d of the pool" % (
        cid, bad.size, "c's polynomials" if kept else "the polynomials", bad[0])


def _product_case(inst, policy, ksh, m, nlimbs, batch, options, entry, ptrs=False, lazy=False, suffix=""):
    """entry "mul": both operands as coefficients (ntt_negacyclic_mul_batch, its RNS twin, or -- ptrs -- the device-table twins);
    "given": ntt_mul_transformed_batch (lazy: NTT_MUL_LAZY_IN with the highest words it admits)"""
    n = 1 << m
    cid = kernel_inventory.case_id(inst) + suffix

    def run(lib, oracle):
        ps = make_plans(lib, oracle, policy, ksh, n, nlimbs)
        try:
            plans, qs = [p for p, _, _ in ps], [q for _, q, _ in ps]
            for p in plans:
                for o, v in options:
                    p.set_option(getattr(lib, o), v)
            if nlimbs > 1:
                lib.set_rns_launch(plans, 0)
            refs = [_product_reference(oracle, cx, n, q, batch, i, entry == "given") for i, (_, q, cx) in enumerate(ps)]
            a, b, want = ([r[k] for r in refs] for k in range(3))
            if lazy:
                b = [_lift_lazy(oracle, x, q, 0x1A2 + i) for i, (x, q) in enumerate(zip(b, qs))]
            # what the header says about the operands: the one-launch forms up to 2^14 leave the coefficient operands as they
            # were; the transformed operand is const; everything else is scratch
            one_launch = m <= 14 and dict(options).get("OPT_FUSED_PRODUCT", 1) == 1
            if ptrs:
                _run_tables(lib, cid, plans, qs, n, batch, a, b, want, kept=one_launch)
            else:
                _run_slab(lib, cid, plans, qs, n, batch, entry, lib.MUL_LAZY_IN if lazy else 0, a, b, want,
                          a_kept=one_launch, b_kept=entry == "given")
        finally:
            for p, _, _ in ps:
                p.destroy()
    return Case(cid, inst, run)


def _grid_option(options, grid, nl):
    """NTT_OPT_MAX_GRID for `grid` workgroups per limb (0: the launch's own grid): block_grid (ntt_kernels_block.h) shares the cap
    among the limbs of a launch, and rns_compatible (host_products.inc) wants it equal on every plan of a run"""
    return options + ((("OPT_MAX_GRID", grid * nl),) if grid else ())


def _product_forms(inst, ksh, m, batch, options, grid, multi, both, ptrs, suffix=""):
    """the cases of one product instance: both operands as coefficients -- one case --, or one operand given transformed --
    canonical and lazy words, the same launch"""
    nl = _nlimbs(multi)
    opts = _grid_option(options, grid, nl)
    if both:
        return [_product_case(inst, inst.policy, ksh, m, nl, batch, opts, "mul", ptrs=ptrs, suffix=suffix)]
    return [_product_case(inst, inst.policy, ksh, m, nl, batch, opts, "given", lazy=lazy, suffix=suffix + ("-lazy" if lazy else ""))
            for lazy in (False, True)]


def _fp2_case(inst, ksh, m, batch, options, grid):
    """NTT_OPT_FUSED_PRODUCT 2: ntt_negacyclic_mul_batch with a's forward transform as a launch of its own (lazy words), then the
    operand-given kernel: the instance ntt_mul_transformed_batch launches, fed by the library's own lazy transform"""
    opts = _grid_option(options + (("OPT_FUSED_PRODUCT", 2),), grid, 1)
    return _product_case(inst, inst.policy, ksh, m, 1, batch, opts, "mul", suffix="-fp2")


def recipe_fused_product(inst):
    """fused_product_kernel<A, LOGN, KSH, ALAZY, WHOLE, MULTI, BOTH, PTRS> (ntt_kernels_launch.h, launch_product_impl /
    launch_product_blocks; host_products.inc, fused_product).
    WHOLE: N = 2^LOGN, two workgroups per limb over 5 polynomials: workgroup 0 takes blocks 0, 2, 4, workgroup 1 blocks 1, 3.
    !WHOLE: the blocks of N = 2^15 with NTT_OPT_BLOCK_LOG = LOGN (12: three, 14: one column stage around the launch) and the
    XCD-local launch off; block_grid rounds the cap up to the 2^s0 blocks of a polynomial, so with 3 polynomials every
    workgroup takes three blocks at its position.  The instance of class 0 of the scheduled policy, one limb, also at the
    largest stage count in front of the blocks (2^16 for 2^12-point blocks, NTT_OPT_BLOCK_LOG's limit; 2^17 for 2^14), and
    the operand-given one once more behind the library's own lazy transform (NTT_OPT_FUSED_PRODUCT 2)."""
    a = inst.args
    ln, whole, multi, both, ptrs = a["LOGN"], a["WHOLE"], a["MULTI"], a["BOTH"], a["PTRS"]
    if not a["ALAZY"] or (ptrs and not (both and whole)) or (ln == 13 and not whole) or ln not in (12, 13, 14):
        return None
    plain = inst.policy == "ArithF64" and a["KSH"] == 0 and not multi and not ptrs
    if whole:
        out = _product_forms(inst, a["KSH"], ln, 5, (), 2, multi, both, ptrs)
        if plain and not both:
            out.append(_fp2_case(inst, a["KSH"], ln, 5, (), 2))
        return out
    opts = (("OPT_BLOCK_LOG", ln), ("OPT_XCD_LOCAL", 0))
    out = _product_forms(inst, a["KSH"], 15, 3, opts, 1, multi, both, ptrs)
    if plain:
        top = 16 if ln == 12 else 17
        out += _product_forms(inst, a["KSH"], top, 3, opts, 1, multi, both, ptrs, suffix="-N%d" % top)[:1]
        if not both:
            out.append(_fp2_case(inst, a["KSH"], 15, 3, opts, 1))
    return out


def small_product_batch(logn):
    """four full groups of BPW = 2^(12 - LOGN) polynomials (ntt_kernels_block.h, Geom: 256 threads, 16 words each) and a fifth with
    more than half of its sub-blocks live, the first dead one in the same wave as a live one where a wave holds several: with
    two workgroups per limb, workgroup 0 wraps twice and ends on the partly dead group, workgroup 1 wraps once"""
    bpw = 1 << (12 - logn)
    return 4 * bpw + (bpw // 2 + 1 if bpw >= 4 else 1)


def recipe_fused_product_small(inst):
    """fused_product_small_kernel<A, LOGN, KSH, MULTI, BOTH, PTRS>: N = 2^LOGN, 8..11 (launch_product_blocks), tables filled once
    per workgroup; batch: small_product_batch"""
    a = inst.args
    ln, multi, both, ptrs = a["LOGN"], a["MULTI"], a["BOTH"], a["PTRS"]
    if (ptrs and not both) or not 8 <= ln <= 11:
        return None
    out = _product_forms(inst, a["KSH"], ln, small_product_batch(ln), (), 2, multi, both, ptrs)
    if inst.policy == "ArithF64" and a["KSH"] == 0 and not multi and not both:
        out.append(_fp2_case(inst, a["KSH"], ln, small_product_batch(ln), (), 2))
    return out


def recipe_team_product(inst):
    """team_product_kernel<A, LEAD, KSH, FOUR, MULTI, PTRS>: N = 2^(12 + LEAD), NTT_OPT_XCD_LOCAL 1, 65 polynomials (two limbs:
    33 each) -- one past the 64 polynomials x limbs of team_applies (host_transforms.inc) and ptrs_team (host_ntt_domain.inc).
    FOUR: ntt_negacyclic_mul_batch (fused_product: four = !ahat_given); !FOUR: ntt_mul_transformed_batch.  The launch is
    1024 workgroups on eight queues (team_prologue): every workgroup pulls items until its queue is empty."""
    a = inst.args
    four, multi, ptrs = a["FOUR"], a["MULTI"], a["PTRS"]
    if (ptrs and not four) or not 3 <= a["LEAD"] <= 5:
        return None
    return _product_forms(inst, a["KSH"], 12 + a["LEAD"], 33 if multi else 65, (("OPT_XCD_LOCAL", 1),), 0, multi, four, ptrs)


# --------------------------------------------------------------------------------------------------------------------
# pointwise kernels (host_products.inc, host_ntt_domain.inc): the policy follows the plan's arithmetic alone
# --------------------------------------------------------------------------------------------------------------------
PW_LOGN, PW_BATCH, PW_GRID = 10, 5, 8   # 20 blocks of 256 words on 8 workgroups (grid_pw): four of them loop three times, four twice


def _pw_plan(lib, oracle, policy):
    """the largest prime the policy's plans accept: FP64 plans go up to 52 bits (the class of ArithF64W: pointwise_launch takes
    ArithF64 for every FP64 plan), the reference's integer butterflies to 61"""
    n = 1 << PW_LOGN
    arith = lib.ARITH_U64 if policy == "ArithU64" else lib.ARITH_AUTO
    q = prime_for(lib, "ArithU64" if policy == "ArithU64" else "ArithF64W", 0, n)
    w = lib.min_root(q, n)
    plan = lib.Plan(n, q, w, arith=arith)
    plan.set_option(lib.OPT_MAX_GRID, PW_GRID)
    return plan, q, oracle.ctx(n, q, w)


def _pw_operand(oracle, n, q, batch, seed, lazy, fifth):
    """(residues, words handed to the kernel): inputs() with word 5 as given and -- of a whole batch -- the last polynomial q-1
    throughout; lazy: lifted anywhere into [0,4q), the first eight words by 3q -- word 2 is 4q-1"""
    r = inputs(oracle, n, q, batch, seed)
    if batch > 1:
        r[-n:] = np.uint64(q - 1)
    r[5] = np.uint64(fifth)
    if not lazy:
        return r, r
    w = r + np.uint64(q) * oracle.fill_uniform(r.size, 4, seed ^ 0x55)
    w[:8] = r[:8] + np.uint64(3 * q)
    assert int(w[2]) == 4 * q - 1 and int(w.max()) < 4 * q
    return r, w


def _pw_case(inst, form):
    """form "mul": ntt_pointwise_mul_batch(_lazy); "dot": ntt_inv_dot_batch with NTT_OPT_DOT_FUSED 0 -- pointwise_acc_kernel per
    pair, accumulating from the second on, then the inverse transform; "ptrs": ntt_inv_dot_dev_ptrs likewise
    (pointwise_ptrs_kernel; BCAST: every b is ONE polynomial shared by the batch)"""
    a_ = inst.args
    lazy, acc, bcast = a_["LAZYIN"], a_.get("ACC", False), a_.get("BCAST", False)
    n, batch = 1 << PW_LOGN, PW_BATCH
    cid = kernel_inventory.case_id(inst)

    def run(lib, oracle):
        plan, q, cx = _pw_plan(lib, oracle, inst.policy)
        bufs = []
        try:
            if form != "mul":
                plan.set_option(lib.OPT_DOT_FUSED, 0)
            k = 2 if acc else 1
            # word 5: (q-1) * 1 in the first pair and 1 * (q-1) in the second: c = q-1 on entry of the accumulating launch, the
            # product q-1 again, c + t = 2q-2
            ar, aw = zip(*[_pw_operand(oracle, n, q, batch, 0xA11 + i, lazy, (q - 1, 1)[i]) for i in range(k)])
            br, bw = zip(*[_pw_operand(oracle, n, q, 1 if bcast else batch, 0xB22 + i, lazy, (1, q - 1)[i]) for i in range(k)])
            prod = oracle.dot(list(ar), list(br), q, N=n, bcast=bcast)
            want = prod if form == "mul" else cx.inv(prod)
            assert int(want.max()) < q
            if form == "ptrs":
                got = _pw_tables(lib, cid, plan, n, batch, aw, bw, bcast, lazy)
            else:
                da = [lib.DeviceBuffer(x.size).upload(x) for x in aw]
                db = [lib.DeviceBuffer(x.size).upload(x) for x in bw]
                ic = np.full(batch * n + n, GUARD, dtype=np.uint64)
                dc = lib.DeviceBuffer(ic.size).upload(ic)
                bufs += da + db + [dc]
                if form == "mul":
                    plan.pointwise_mul(dc.ptr, da[0].ptr, db[0].ptr, batch, lazy_in=lazy)
                else:
                    plan.inv_dot(dc.ptr, [d.ptr for d in da], [d.ptr for d in db], batch,
                                 (lib.MUL_LAZY_IN if lazy else 0) | (lib.MUL_B_BROADCAST if bcast else 0))
                got = dc.download()
                assert (got[batch * n:] == GUARD).all(), "%s: the polynomial behind the output was written" % cid
                for what, d, w in [("a", d, w) for d, w in zip(da, aw)] + [("b", d, w) for d, w in zip(db, bw)]:
                    assert np.array_equal(d.download(), w), "%s: a const operand (%s) was written" % (cid, what)
                got = got[:batch * n]
            _assert_words(cid, "c", got, want, n, 0, q)
        finally:
            for d in bufs:
                d.free()
            plan.destroy()
    return Case(cid, inst, run)


def _pw_tables(lib, cid, plan, n, batch, aw, bw, bcast, lazy):
    """c and every operand polynomial at a place of its own in one pool (shuffled, irregular gaps), handed over as device tables;
    a broadcast b as a device pointer to its one polynomial.  Returns c's polynomials in order."""
    k = len(aw)
    nb = 1 if bcast else batch
    rng = np.random.default_rng(0x9017 + k)
    total = batch * (1 + k) + nb * k
    gaps = rng.integers(1, 40, size=total) + np.arange(total) % 7
    starts = np.cumsum(gaps + n) - n
    words = int(starts[-1] + 2 * n)
    offs = starts[rng.permutation(total)]
    oc, oa, ob = offs[:batch], offs[batch:batch * (1 + k)].reshape(k, batch), offs[batch * (1 + k):].reshape(k, nb)
    img = np.full(words, GUARD, dtype=np.uint64)
    for i in range(k):
        for p in range(batch):
            img[int(oa[i][p]):int(oa[i][p]) + n] = aw[i][p * n:(p + 1) * n]
        for p in range(nb):
            img[int(ob[i][p]):int(ob[i][p]) + n] = bw[i][p * n:(p + 1) * n]
    pool = lib.DeviceBuffer(words).upload(img)

    def table(o):
        return lib.DeviceBuffer(len(o)).upload(np.uint64(pool.ptr) + np.uint64(8) * o.astype(np.uint64))
    tc, ta = table(oc), [table(oa[i]) for i in range(k)]
    tb = [] if bcast else [table(ob[i]) for i in range(k)]
    try:
        bs = [pool.ptr + 8 * int(ob[i][0]) for i in range(k)] if bcast else [t.ptr for t in tb]
        plan.inv_dot_dev_ptrs(tc.ptr, [t.ptr for t in ta], bs, batch, (lib.MUL_LAZY_IN if lazy else 0) | (lib.MUL_B_BROADCAST if bcast else 0))
        got = pool.download()
    finally:
        pool.free()
        for t in [tc] + ta + tb:
            t.free()
    out = np.zeros(words, dtype=bool)
    for p in range(batch):
        out[int(oc[p]):int(oc[p]) + n] = True
    bad = np.nonzero(~out & (got != img))[0]
    assert bad.size == 0, "%s: %d words outside c's polynomials were written, first at word %d of the pool" % (cid, bad.size, bad[0])
    return np.concatenate([got[int(o):int(o) + n] for o in oc])


def _pw_policy(inst):
    return inst.policy in ("ArithF64", "ArithU64")


def recipe_pointwise(inst):
    """pointwise_kernel<A, LAZYIN>: ntt_pointwise_mul_batch / ntt_pointwise_mul_batch_lazy (host_products.inc, pointwise_launch)"""
    return [_pw_case(inst, "mul")] if _pw_policy(inst) else None


def recipe_pointwise_acc(inst):
    """pointwise_acc_kernel<A, LAZYIN, ACC>: ntt_inv_dot_batch on a plan with NTT_OPT_DOT_FUSED 0 (host_ntt_domain.inc, inv_dot:
    !dot_kernel_applies), one pair (ACC false) or two (the second launch accumulates)"""
    return [_pw_case(inst, "dot")] if _pw_policy(inst) else None


def recipe_pointwise_ptrs(inst):
    """pointwise_ptrs_kernel<A, LAZYIN, ACC, BCAST>: ntt_inv_dot_dev_ptrs on a plan with NTT_OPT_DOT_FUSED 0 (host_ntt_domain.inc,
    inv_dot_ptrs_limb -> pointwise_ptrs)"""
    return [_pw_case(inst, "ptrs")] if _pw_policy(inst) else None


RECIPES = {
    "onepass_kernel": recipe_onepass,
    "twophase_kernel": recipe_twophase,
    "team_kernel": recipe_team,
    "column_kernel": recipe_column,
    "fused_product_kernel": recipe_fused_product,
    "fused_product_small_kernel": recipe_fused_product_small,
    "team_product_kernel": recipe_team_product,
    "pointwise_kernel": recipe_pointwise,
    "pointwise_acc_kernel": recipe_pointwise_acc,
    "pointwise_ptrs_kernel": recipe_pointwise_ptrs,
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
    verbose = "--times" in argv
    argv = [x for x in argv if x != "--times"]
    if argv and argv[0] == "--family":
        assert len(argv) == 2 and argv[1] in RECIPES, "--family takes one of: %s" % ", ".join(RECIPES)
        sel = [c for c in cases() if c.inst.family == argv[1]]
    else:
        sel = [c for c in cases() if not argv or any(s in c.id for s in argv)]
    t0, failed = time.time(), []
    for c in sel:
        t1 = time.time()
        try:
            c.run(lib, oracle)
        except AssertionError as e:
            failed.append((c.id, str(e)))
            print("FAIL", c.id, e, flush=True)
        if verbose:
            print("%7.2f s  %s" % (time.time() - t1, c.id), flush=True)
    print("ran %d cases in %.1f s, %d failed" % (len(sel), time.time() - t0, len(failed)), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
