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

The NTT-domain product families (dot_inv_kernel, team_dot_kernel: c = inv(sum_i a_i^ (.) b_i^); fwd_mul_kernel, team_mul_kernel,
onepass_mul_kernel: c^ = fwd(a) (.) b^ (+ c^)) are driven through ntt_inv_dot_batch / ntt_fwd_mul_batch, their strided RNS twins on
the padded limb-major layout (MULTI) and the device-pointer-table twins (PTRS; a broadcast b^ a dense [limb][N] polynomial).  Flags
are run-time fields, so every instance gets two cases: one pair (store) of canonical words with one b^ per polynomial, and
kDotEvery + 1 pairs (accumulate) of lazy words with a broadcast b^.  Fixed words of the first polynomial carry the extremes:
(q-1) x (q-1), the residue q-1 in every term (the running sum at its largest in front of a fold), 4q-1 x 4q-1 and q-1 carried as
4q-1 among the lazy words; b^ = q-1, b^ = 0 and c^ = q-1 on top of a product q-1 in the mul forms.  The batch comes from the
geometry these kernels are launched with (domain_batch), the grid is capped as for the product families.  Once per policy and class
the slab form of dot_inv_kernel at 2^6 and 2^14 runs k = kDotEvery, kDotEvery + 1 and 32 pairs, canonical and lazy; team_dot_kernel
once per policy 32 lazy pairs; once per family and policy c aliases an operand where the header allows it.  The references are
checked against schoolbook products by tests/test_domain_reference_cpu.py.

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

import kernel_inventory  # noqa: E402
import rns_support as rs  # noqa: E402

# instances no recipe covers yet, one normalised key per line: fused_kernel and the plain host kernels.  Pinned so that a new instantiation in any family fails
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


# one operand of a call: data = its words per limb ([batch][N], or -- shared -- ONE polynomial of N words: a broadcast b^, handed over
# dense as [limb][N]); kept: the header declares it const or "left as it was", so every word must come back unchanged (otherwise
# it is scratch: only the words outside its polynomials stay)
Op = collections.namedtuple("Op", "name data kept shared")


def _run_slab(lib, cid, plans, qs, n, batch, ins, want, call, c_init=None, alias=None):
    """the operands as slabs in _slab_layout; call(dc, [device buffer of every operand], layout) issues the entry point;
    c_init: what c holds on entry (accumulating forms), alias: index of the operand whose buffer is handed over as c"""
    nl = len(plans)
    lay = _slab_layout(n, nl, batch)
    imgs = [np.concatenate(list(op.data) + [np.full(n, GUARD, dtype=np.uint64)]) if op.shared else _slab_image(op.data, n, batch, lay)
            for op in ins]
    ic = imgs[alias] if alias is not None else (
        np.full(lay[2], GUARD, dtype=np.uint64) if c_init is None else _slab_image(c_init, n, batch, lay))
    bufs = [lib.DeviceBuffer(x.size).upload(x) for x in imgs]
    dc = bufs[alias] if alias is not None else lib.DeviceBuffer(lay[2]).upload(ic)
    try:
        call(dc, bufs, lay)
        got, gc = [d.download() for d in bufs], dc.download()
    finally:
        for d in bufs + ([] if alias is not None else [dc]):
            d.free()
    for l, g in enumerate(_slab_polys(gc, n, nl, batch, lay)):
        _assert_words(cid, "c", g, want[l], n, l, qs[l])
    _assert_unwritten(cid, "c", gc, ic, n, nl, batch, lay)
    for i, (op, g, before) in enumerate(zip(ins, got, imgs)):
        if i == alias:
            continue
        if op.kept or op.shared:
            assert np.array_equal(g, before), "%s: operand %s was written (the header leaves it as it was)" % (cid, op.name)
        else:
            _assert_unwritten(cid, op.name, g, before, n, nl, batch, lay)


def _run_tables(lib, cid, plans, qs, n, count, ins, want, call, c_init=None):
    """the operands and c as device tables of `count` pointers into one pool: every polynomial (RNS: its limbs, n + 16 words
    apart behind the entry) at a place of its own, the operands interleaved, shuffled, no two gaps alike -- a kernel that
    computes slab offsets instead of reading the tables produces wrong words.  A shared operand (a broadcast b^) is no table: its
    [limb][N] words lie behind the records, and the call gets their device address.  call([table or address of every operand],
    c's table, limb stride) issues the entry point."""
    nl = len(plans)
    lstride = n + 16
    rec = (nl - 1) * lstride + n
    tabbed = [i for i, op in enumerate(ins) if not op.shared]
    nt = len(tabbed) + 1
    rng = np.random.default_rng(0x7AB1E + n + count)
    gaps = rng.integers(1, 40, size=nt * count) + np.arange(nt * count) % 7
    starts = np.cumsum(gaps + rec) - rec
    end = int(starts[-1] + rec)
    shared_at = {i: end + 24 + j * (nl * n + 24) for j, i in enumerate(i for i, op in enumerate(ins) if op.shared)}
    words = end + len(shared_at) * (nl * n + 24) + n
    offs = starts[rng.permutation(nt * count)].reshape(nt, count)
    img = np.full(words, GUARD, dtype=np.uint64)
    for o, src in [(o, ins[i].data) for o, i in enumerate(tabbed)] + ([(nt - 1, c_init)] if c_init is not None else []):
        for l in range(nl):
            for p in range(count):
                at = int(offs[o][p]) + l * lstride
                img[at:at + n] = src[l][p * n:(p + 1) * n]
    for i, at in shared_at.items():
        img[at:at + nl * n] = np.concatenate(list(ins[i].data))
    pool = lib.DeviceBuffer(words).upload(img)
    tabs = [lib.DeviceBuffer(count).upload((np.uint64(pool.ptr) + np.uint64(8) * offs[o].astype(np.uint64))) for o in range(nt)]
    try:
        args = [pool.ptr + 8 * shared_at[i] if op.shared else tabs[tabbed.index(i)].ptr for i, op in enumerate(ins)]
        call(args, tabs[nt - 1].ptr, lstride)
        got = pool.download()
    finally:
        pool.free()
        for t in tabs:
            t.free()
    written = np.zeros(words, dtype=bool)
    scratch = [o for o, i in enumerate(tabbed) if not ins[i].kept]
    for l in range(nl):
        g = np.concatenate([got[int(offs[nt - 1][p]) + l * lstride:int(offs[nt - 1][p]) + l * lstride + n] for p in range(count)])
        _assert_words(cid, "c", g, want[l], n, l, qs[l])
        for o in [nt - 1] + scratch:   # (scratch operands: only what lies between the polynomials stays)
            for p in range(count):
                at = int(offs[o][p]) + l * lstride
                written[at:at + n] = True
    bad = np.nonzero(~written & (got != img))[0]
    assert bad.size == 0, "%s: %d words outside %s were written, first at word %d of the pool" % (
        cid, bad.size, "the polynomials of c and of %s" % ", ".join(ins[tabbed[o]].name for o in scratch) if scratch else "c's polynomials", bad[0])


def _apply(lib, plans, options):
    for p in plans:
        for o, v in options:
            p.set_option(getattr(lib, o), v)
    if len(plans) > 1:
        lib.set_rns_launch(plans, 0)


def _product_case(inst, policy, ksh, m, nlimbs, batch, options, entry, ptrs=False, lazy=False, suffix=""):
    """entry "mul": both operands as coefficients (ntt_negacyclic_mul_batch, its RNS twin, or -- ptrs -- the device-table twins);
    "given": ntt_mul_transformed_batch (lazy: NTT_MUL_LAZY_IN with the highest words it admits)"""
    n = 1 << m
    cid = kernel_inventory.case_id(inst) + suffix

    def run(lib, oracle):
        ps = make_plans(lib, oracle, policy, ksh, n, nlimbs)
        try:
            plans, qs = [p for p, _, _ in ps], [q for _, q, _ in ps]
            _apply(lib, plans, options)
            refs = [_product_reference(oracle, cx, n, q, batch, i, entry == "given") for i, (_, q, cx) in enumerate(ps)]
            a, b, want = ([r[k] for r in refs] for k in range(3))
            if lazy:
                b = [_lift_lazy(oracle, x, q, 0x1A2 + i) for i, (x, q) in enumerate(zip(b, qs))]
            # what the header says about the operands: the one-launch forms up to 2^14 leave the coefficient operands as they
            # were; the transformed operand is const; everything else is scratch
            one_launch = m <= 14 and dict(options).get("OPT_FUSED_PRODUCT", 1) == 1
            flags = lib.MUL_LAZY_IN if lazy else 0
            if ptrs:
                def call(t, ctab, lstride):
                    if nlimbs == 1:
                        plans[0].negacyclic_mul_dev_ptrs(ctab, t[0], t[1], batch)
                    else:
                        lib.rns_negacyclic_mul_dev_ptrs(plans, ctab, t[0], t[1], batch, lstride)
                _run_tables(lib, cid, plans, qs, n, batch, [Op("a", a, one_launch, False), Op("b", b, one_launch, False)], want, call)
            else:
                def call(dc, d, lay):
                    if nlimbs == 1 and entry == "mul":
                        plans[0].negacyclic_mul(dc.ptr, d[0].ptr, d[1].ptr, batch)
                    elif nlimbs == 1:
                        plans[0].mul_transformed(dc.ptr, d[0].ptr, d[1].ptr, batch, flags)
                    elif entry == "mul":
                        lib.rns_negacyclic_mul(plans, dc.ptr, d[0].ptr, d[1].ptr, batch, layout=lay[:2])
                    else:
                        lib.rns_mul_transformed(plans, dc.ptr, d[0].ptr, d[1].ptr, batch, flags, layout=lay[:2])
                _run_slab(lib, cid, plans, qs, n, batch, [Op("a", a, one_launch, False), Op("b", b, entry == "given", False)], want, call)
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
# products of operands in the NTT domain: c = inv(sum_i a_i^ (.) b_i^) (dot_inv_kernel, team_dot_kernel) and
# c^ = fwd(a) (.) b^ (+ c^) (fwd_mul_kernel, team_mul_kernel, onepass_mul_kernel)
# --------------------------------------------------------------------------------------------------------------------
K_MAX_DOT = 32   # kMaxDot (ntt_kernels_products.h)
# words of the first polynomial that carry the extreme values (behind the canonical extremes inputs() puts into words 0..4)
W_SQUARE, W_TOP, W_LAZY, W_CARRY, W_ZERO = 8, 9, 10, 11, 12


def dot_every(policy):
    """kDotEvery of the policy (ntt_arith.h): the terms between two folds of the running sum; None: ArithU64 never folds"""
    return {"ArithF64": 3, "ArithF64W": 1, "ArithU64X<0>": 1, "ArithU64X<1>": 4, "ArithU64X<3>": 20, "ArithU64": None}[policy]


def domain_bpw(policy, logn, inverse):
    """blocks per workgroup of Geom<LOGN, INV, flavor_of<A>()> (ntt_kernels_block.h), the geometry dot_inv_kernel (INV) and
    fwd_mul_kernel (!INV) are launched with: Plan<LOGN>::T = 2^(LOGN - 4) threads per block, 256 / T blocks in a 256-thread
    workgroup below 2^12, one block above -- but two (PERSIST2) in the forward 2^13 kernel of the FP64 policies (flavor 1)"""
    if logn == 13 and not inverse and policy in ("ArithF64", "ArithF64W"):
        return 2
    return max(1, 256 >> (logn - 4))


def domain_batch(policy, logn, inverse):
    """small_product_batch for the geometry of the dot and mul kernels (domain_bpw): four full groups of BPW polynomials and a
    fifth that is partly dead where BPW > 1 (more than half of its sub-blocks live from BPW = 4 on, one of two at BPW = 2); with
    two workgroups per limb (NTT_OPT_MAX_GRID) workgroup 0 takes groups 0, 2, 4 -- it wraps twice and ends on the partly dead
    group -- and workgroup 1 groups 1, 3.  BPW = 1 (2^12 on): five polynomials, blocks 0, 2, 4 and 1, 3."""
    bpw = domain_bpw(policy, logn, inverse)
    return 4 * bpw + (bpw // 2 + 1 if bpw >= 4 else 1)


def _cached(key, make):
    """references of the NTT-domain cases, computed once and shared read-only by the cases on the same operands (the forms of
    one instance, the MULTI / PTRS instances beside it); the cache is bounded by words, the large team cases evict one another"""
    if key in _ref_cache:
        _ref_cache.move_to_end(key)
        return _ref_cache[key]
    _ref_cache[key] = make()
    size = lambda v: sum(x.size for part in v for x in (part if isinstance(part, list) else [part]) if x is not None)  # noqa: E731
    while len(_ref_cache) > 1 and (len(_ref_cache) > 6 or sum(size(v) for v in _ref_cache.values()) > (1 << 28)):
        _ref_cache.popitem(last=False)
    return _ref_cache[key]


def _lift(oracle, r, q, seed, top):
    """the residues r as lazy words anywhere in [0,4q); top: {word: multiple of q added there}"""
    w = r + np.uint64(q) * oracle.fill_uniform(r.size, 4, seed)
    for at, mult in top.items():
        w[at] = r[at] + np.uint64(mult * q)
    assert int(w.max()) < 4 * q and np.array_equal(w % np.uint64(q), r)
    return w


def dot_reference(oracle, cx, n, q, batch, limb, k, lazy, bcast):
    """([a_i^ words], [b_i^ words], want) of one limb: want = inv(sum_{i<k} a_i^ (.) b_i^ mod q), the products by oracle.pointwise
    and an exact modular sum (oracle.dot), the inverse by the oracle.  Every operand is inputs(); in every term the first
    polynomial holds (q-1) x (q-1) at W_SQUARE and (q-1) x 1 at W_TOP (the residue q-1 in every term: the running sum as large
    as it gets in front of a fold), and the last polynomial of every a_i^ and b_i^ is q-1 throughout.  lazy: the words handed
    over are lifted anywhere into [0,4q) (the range ntt_inv_dot_batch admits with NTT_MUL_LAZY_IN: no 2^53 bound there), at
    W_LAZY both factors 4q-1 (the highest lazy word), at W_CARRY the residue q-1 carried as 4q-1 times 1 carried as 3q+1.
    bcast: every b_i^ is one polynomial."""
    def make():
        nb = 1 if bcast else batch
        ar = [inputs(oracle, n, q, batch, 0xA500 + 131 * limb + i) for i in range(k)]
        br = [inputs(oracle, n, q, nb, 0xB600 + 137 * limb + i) for i in range(k)]
        for a, b in zip(ar, br):
            a[-n:] = np.uint64(q - 1)
            if not bcast:
                b[-n:] = np.uint64(q - 1)
            for at, (x, y) in {W_SQUARE: (q - 1, q - 1), W_TOP: (q - 1, 1), W_LAZY: (q - 1, q - 1), W_CARRY: (q - 1, 1)}.items():
                a[at], b[at] = np.uint64(x), np.uint64(y)
        want = cx.inv(oracle.dot(ar, br, q, N=n, bcast=bcast))
        assert int(want.max()) < q
        if lazy:
            aw = [_lift(oracle, a, q, 0x1A2 + i, {W_LAZY: 3, W_CARRY: 3}) for i, a in enumerate(ar)]
            bw = [_lift(oracle, b, q, 0x2B3 + i, {W_LAZY: 3, W_CARRY: 3}) for i, b in enumerate(br)]
            assert int(aw[0][W_LAZY]) == 4 * q - 1 and int(bw[0][W_LAZY]) == 4 * q - 1 and int(bw[0][W_CARRY]) == 3 * q + 1
        else:
            aw, bw = ar, br
        _readonly(want, *aw, *bw)
        return aw, bw, want
    return _cached(("dot", n, q, batch, limb, k, lazy, bcast), make)


def mul_reference(oracle, cx, n, q, batch, limb, lazy, bcast, acc):
    """(a, b^ words, c^ on entry or None, want) of one limb: want = fwd(a) (.) b^ (+ c^) mod q by the oracle.  a: inputs(), its last
    polynomial q-1 throughout; b^: a transformed polynomial with q-1 at W_SQUARE, 0 at W_TOP, q-1 again at W_LAZY -- lazy: carried
    as 4q-1, the highest word NTT_MUL_LAZY_IN admits here, the other words lifted anywhere into [0,4q) -- and at W_CARRY the word
    that makes the product q-1 there; acc: c^ canonical on entry, q-1 at W_CARRY (q-1 + q-1) and 0 at W_ZERO.  The fixed words
    sit in the first polynomial (bcast: b^ is one polynomial, so its fixed words meet every polynomial of a)."""
    def make():
        a = inputs(oracle, n, q, batch, 0x2468 + 17 * limb)
        a[-n:] = np.uint64(q - 1)
        fa = cx.fwd(a)
        nb = 1 if bcast else batch
        br = cx.fwd(inputs(oracle, n, q, nb, 0xB0B + 29 * limb))
        assert int(fa[W_CARRY]) != 0
        for at, v in {W_SQUARE: q - 1, W_TOP: 0, W_LAZY: q - 1, W_CARRY: (q - 1) * pow(int(fa[W_CARRY]), -1, q) % q}.items():
            br[at] = np.uint64(v)
        want = oracle.pointwise(fa, np.tile(br, batch) if bcast else br, q)
        assert int(want[W_CARRY]) == q - 1
        c0 = None
        if acc:
            c0 = oracle.fill_uniform(batch * n, q, 0xC0C + 31 * limb)
            c0[W_CARRY], c0[W_ZERO] = np.uint64(q - 1), np.uint64(0)
            want = (want + c0) % np.uint64(q)
            _readonly(c0)
        bw = _lift(oracle, br, q, 0x3C4, {W_LAZY: 3}) if lazy else br
        _readonly(a, bw, want)
        return a, bw, c0, want
    return _cached(("mul", n, q, batch, limb, lazy, bcast, acc), make)


def _dot_case(inst, ksh, m, nlimbs, batch, options, k, lazy=False, bcast=False, ptrs=False, alias=False, suffix=""):
    """ntt_inv_dot_batch, ntt_rns_inv_dot_batch_strided (nlimbs > 1), ntt_inv_dot_dev_ptrs / ntt_rns_inv_dot_dev_ptrs (ptrs);
    alias: k = 1 and d_c = d_ahat[0], which the header allows.  Every a_i^ and b_i^ is const and must come back unchanged."""
    n = 1 << m
    cid = kernel_inventory.case_id(inst) + suffix

    def run(lib, oracle):
        ps = make_plans(lib, oracle, inst.policy, ksh, n, nlimbs)
        try:
            plans, qs = [p for p, _, _ in ps], [q for _, q, _ in ps]
            _apply(lib, plans, options)
            refs = [dot_reference(oracle, cx, n, q, batch, l, k, lazy, bcast) for l, (_, q, cx) in enumerate(ps)]
            ins = [Op("a%d^" % i, [r[0][i] for r in refs], True, False) for i in range(k)]
            ins += [Op("b%d^" % i, [r[1][i] for r in refs], True, bcast) for i in range(k)]
            want = [r[2] for r in refs]
            flags = (lib.MUL_LAZY_IN if lazy else 0) | (lib.MUL_B_BROADCAST if bcast else 0)
            if ptrs:
                def call(t, ctab, lstride):
                    if nlimbs == 1:
                        plans[0].inv_dot_dev_ptrs(ctab, t[:k], t[k:], batch, flags)
                    else:
                        lib.rns_inv_dot_dev_ptrs(plans, ctab, t[:k], t[k:], batch, lstride, flags)
                _run_tables(lib, cid, plans, qs, n, batch, ins, want, call)
            else:
                def call(dc, d, lay):
                    pa, pb = [x.ptr for x in d[:k]], [x.ptr for x in d[k:]]
                    if nlimbs == 1:
                        plans[0].inv_dot(dc.ptr, pa, pb, batch, flags)
                    else:
                        lib.rns_inv_dot(plans, dc.ptr, pa, pb, batch, flags, layout=lay[:2])
                _run_slab(lib, cid, plans, qs, n, batch, ins, want, call, alias=0 if alias else None)
        finally:
            for p, _, _ in ps:
                p.destroy()
    return Case(cid, inst, run)


def _mul_case(inst, ksh, m, nlimbs, batch, options, lazy=False, bcast=False, acc=False, ptrs=False, a_kept=True, alias=None, suffix=""):
    """ntt_fwd_mul_batch, ntt_rns_fwd_mul_batch_strided (nlimbs > 1), ntt_fwd_mul_dev_ptrs / ntt_rns_fwd_mul_dev_ptrs (ptrs); alias:
    d_c = d_a (0) or d_bhat (1), store form.  b^ is const; a_kept: the header leaves a as it was (up to 2^14, and 2^15 in one pass)."""
    n = 1 << m
    cid = kernel_inventory.case_id(inst) + suffix

    def run(lib, oracle):
        ps = make_plans(lib, oracle, inst.policy, ksh, n, nlimbs)
        try:
            plans, qs = [p for p, _, _ in ps], [q for _, q, _ in ps]
            _apply(lib, plans, options)
            refs = [mul_reference(oracle, cx, n, q, batch, l, lazy, bcast, acc) for l, (_, q, cx) in enumerate(ps)]
            ins = [Op("a", [r[0] for r in refs], a_kept, False), Op("b^", [r[1] for r in refs], True, bcast)]
            c0, want = [r[2] for r in refs] if acc else None, [r[3] for r in refs]
            flags = (lib.MUL_LAZY_IN if lazy else 0) | (lib.MUL_B_BROADCAST if bcast else 0) | (lib.MUL_ACCUMULATE if acc else 0)
            if ptrs:
                def call(t, ctab, lstride):
                    if nlimbs == 1:
                        plans[0].fwd_mul_dev_ptrs(ctab, t[0], t[1], batch, flags)
                    else:
                        lib.rns_fwd_mul_dev_ptrs(plans, ctab, t[0], t[1], batch, lstride, flags)
                _run_tables(lib, cid, plans, qs, n, batch, ins, want, call, c_init=c0)
            else:
                def call(dc, d, lay):
                    if nlimbs == 1:
                        plans[0].fwd_mul(dc.ptr, d[0].ptr, d[1].ptr, batch, flags)
                    else:
                        lib.rns_fwd_mul(plans, dc.ptr, d[0].ptr, d[1].ptr, batch, flags, layout=lay[:2])
                _run_slab(lib, cid, plans, qs, n, batch, ins, want, call, c_init=c0, alias=alias)
        finally:
            for p, _, _ in ps:
                p.destroy()
    return Case(cid, inst, run)


def _dot_forms(inst, ksh, m, nl, batch, opts, ptrs, suffix=""):
    """the two cases of every dot instance: one pair of canonical words, one b^ per polynomial; kDotEvery + 1 pairs (the first
    term behind a fold; 3 for ArithU64, which never folds) of lazy words with broadcast b^"""
    every = dot_every(inst.policy)
    return [_dot_case(inst, ksh, m, nl, batch, opts, 1, ptrs=ptrs, suffix=suffix),
            _dot_case(inst, ksh, m, nl, batch, opts, every + 1 if every else 3, lazy=True, bcast=True, ptrs=ptrs, suffix=suffix + "-lazy-bcast")]


def _mul_forms(inst, ksh, m, nl, batch, opts, ptrs, a_kept, suffix=""):
    """the two cases of every mul instance: store, canonical words, one b^ per polynomial; accumulate onto c^, lazy words,
    broadcast b^"""
    return [_mul_case(inst, ksh, m, nl, batch, opts, ptrs=ptrs, a_kept=a_kept, suffix=suffix),
            _mul_case(inst, ksh, m, nl, batch, opts, lazy=True, bcast=True, acc=True, ptrs=ptrs, a_kept=a_kept, suffix=suffix + "-acc-lazy-bcast")]


def _first_class(inst):
    """one instance per policy: of the scheduled FP64 policy class 0 (the other policies have one class each)"""
    return inst.policy != "ArithF64" or inst.args["KSH"] == 0


def recipe_dot_inv(inst):
    """dot_inv_kernel<A, LOGN, KSH, LASTINV, MULTI, PTRS> (ntt_kernels_launch.h, launch_dot_impl / launch_dot_blocks;
    host_ntt_domain.inc, inv_dot, rns_inv_dot, inv_dot_ptrs_limb / inv_dot_ptrs_run).
    LASTINV: N = 2^LOGN, 6..14 (launch_dot_impl: with_int<6, 14>), ntt_inv_dot_batch; MULTI: ntt_rns_inv_dot_batch_strided with
    NTT_OPT_RNS_LAUNCH 0 (rns_one_launch_pays); PTRS: ntt_inv_dot_dev_ptrs (ptrs_fused), with MULTI ntt_rns_inv_dot_dev_ptrs
    (ptrs_run_pays).  Batch: domain_batch for Geom<LOGN, true, flavor>, two workgroups per limb.
    !LASTINV (launch_dot_impl: logn > kFusedMax, block_log 12 or 14; no PTRS form): the blocks of N = 2^15 with
    NTT_OPT_BLOCK_LOG = LOGN, the XCD-local launch off, 3 polynomials; block_grid rounds the cap of one workgroup up to the 2^s0
    blocks of a polynomial, so every workgroup takes three blocks at its position.
    Once per policy and class, slab form, LOGN 6 and 14: k = kDotEvery, kDotEvery + 1 and 32 pairs, canonical and lazy words
    (ArithU64 never folds: 32).  Once per policy (LOGN 12): k = 1 with d_c = d_ahat[0]."""
    a = inst.args
    ln, ksh, multi, ptrs = a["LOGN"], a["KSH"], a["MULTI"], a["PTRS"]
    nl = _nlimbs(multi)
    if not a["LASTINV"]:
        if ptrs or ln not in (12, 14):
            return None
        opts = _grid_option((("OPT_BLOCK_LOG", ln), ("OPT_XCD_LOCAL", 0)), 1, nl)
        return _dot_forms(inst, ksh, 15, nl, 3, opts, False)
    if not 6 <= ln <= 14:
        return None
    opts, batch = _grid_option((), 2, nl), domain_batch(inst.policy, ln, True)
    out = _dot_forms(inst, ksh, ln, nl, batch, opts, ptrs)
    if not multi and not ptrs:
        if ln in (6, 14):
            every = dot_every(inst.policy)
            for k in sorted({every, every + 1, K_MAX_DOT} if every else {K_MAX_DOT}):
                out += [_dot_case(inst, ksh, ln, 1, batch, opts, k, lazy=lazy, suffix="-k%d%s" % (k, "-lazy" if lazy else ""))
                        for lazy in (False, True)]
        if ln == 12 and _first_class(inst):
            out.append(_dot_case(inst, ksh, ln, 1, batch, opts, 1, alias=True, suffix="-alias-a"))
    return out


def recipe_fwd_mul(inst):
    """fwd_mul_kernel<A, LOGN, KSH, MULTI, PTRS> (ntt_kernels_launch.h, launch_fwd_mul_impl / launch_fwd_mul_blocks;
    host_ntt_domain.inc, fwd_mul, rns_fwd_mul, fwd_mul_ptrs_limb).  N = 2^LOGN, 6..14 (with_int<6, 14>): ntt_fwd_mul_batch; MULTI:
    ntt_rns_fwd_mul_batch_strided with NTT_OPT_RNS_LAUNCH 0; PTRS: ntt_fwd_mul_dev_ptrs (ptrs_fused), with MULTI
    ntt_rns_fwd_mul_dev_ptrs.  Batch: domain_batch for Geom<LOGN, false, flavor> (two blocks per workgroup at 2^13 with the FP64
    policies), two workgroups per limb.  a is left as it was.
    The instances of LOGN 12 and 14 without PTRS also as the block pass of N = 2^15 (launch_fwd_mul_impl: logn > kFusedMax; s0 != 0):
    NTT_OPT_BLOCK_LOG = LOGN, the XCD-local and the one-pass launch off, 3 polynomials, every workgroup three blocks at its
    position; a is scratch there.  Once per policy (LOGN 12): the store form with d_c = d_a and with d_c = d_bhat."""
    a = inst.args
    ln, ksh, multi, ptrs = a["LOGN"], a["KSH"], a["MULTI"], a["PTRS"]
    if not 6 <= ln <= 14:
        return None
    nl = _nlimbs(multi)
    opts, batch = _grid_option((), 2, nl), domain_batch(inst.policy, ln, False)
    out = _mul_forms(inst, ksh, ln, nl, batch, opts, ptrs, True)
    if ln in (12, 14) and not ptrs:
        blk = _grid_option((("OPT_BLOCK_LOG", ln), ("OPT_XCD_LOCAL", 0), ("OPT_ONE_PASS", 0)), 1, nl)
        out += _mul_forms(inst, ksh, 15, nl, 3, blk, False, False, suffix="-N15")
    if ln == 12 and not multi and not ptrs and _first_class(inst):
        out += [_mul_case(inst, ksh, ln, 1, batch, opts, alias=0, suffix="-alias-a"),
                _mul_case(inst, ksh, ln, 1, batch, opts, alias=1, suffix="-alias-b")]
    return out


def _team_shape(a):
    """N = 2^(12 + LEAD) and 65 polynomials (two limbs: 33 each): one past the 64 polynomials x limbs inv_dot / fwd_mul
    (host_ntt_domain.inc: polys >= 64) and ptrs_team want; NTT_OPT_XCD_LOCAL 1 forces the one-launch form, NTT_OPT_ONE_PASS 0
    keeps 2^15 with the FP64 policies from the one-pass kernel (fwd_mul asks one_pass_pays first)"""
    nl = _nlimbs(a["MULTI"])
    return 12 + a["LEAD"], nl, 33 if nl > 1 else 65, (("OPT_XCD_LOCAL", 1), ("OPT_ONE_PASS", 0))


def recipe_team_dot(inst):
    """team_dot_kernel<A, LEAD, KSH, MULTI, PTRS> (ntt_kernels_launch.h, launch_dot_impl: da.team_ctl -> launch_team_dot;
    host_ntt_domain.inc, inv_dot: team, inv_dot_ptrs_limb: ptrs_team): _team_shape, LEAD 3..5 (with_int<3, 5>).  The launch is the
    team kernels' own grid on eight queues (team_prologue).  Once per policy (LEAD 3, slab): 32 pairs of lazy words, and k = 1
    with d_c = d_ahat[0]."""
    a = inst.args
    if not 3 <= a["LEAD"] <= 5:
        return None
    m, nl, batch, opts = _team_shape(a)
    out = _dot_forms(inst, a["KSH"], m, nl, batch, opts, a["PTRS"])
    if a["LEAD"] == 3 and nl == 1 and not a["PTRS"] and _first_class(inst):
        out += [_dot_case(inst, a["KSH"], m, 1, batch, opts, K_MAX_DOT, lazy=True, suffix="-k32-lazy"),
                _dot_case(inst, a["KSH"], m, 1, batch, opts, 1, alias=True, suffix="-alias-a")]
    return out


def recipe_team_mul(inst):
    """team_mul_kernel<A, LEAD, KSH, MULTI, PTRS> (ntt_kernels_launch.h, launch_fwd_mul_impl: ma.team_ctl -> launch_team_mul;
    host_ntt_domain.inc, fwd_mul: team, fwd_mul_ptrs_limb: ptrs_team): _team_shape, LEAD 3..5; a's column stages run in place, so
    a is scratch.  Once per policy (LEAD 3, slab): the store form with d_c = d_a and with d_c = d_bhat."""
    a = inst.args
    if not 3 <= a["LEAD"] <= 5:
        return None
    m, nl, batch, opts = _team_shape(a)
    out = _mul_forms(inst, a["KSH"], m, nl, batch, opts, a["PTRS"], False)
    if a["LEAD"] == 3 and nl == 1 and not a["PTRS"] and _first_class(inst):
        out += [_mul_case(inst, a["KSH"], m, 1, batch, opts, a_kept=False, alias=0, suffix="-alias-a"),
                _mul_case(inst, a["KSH"], m, 1, batch, opts, a_kept=False, alias=1, suffix="-alias-b")]
    return out


def recipe_onepass_mul(inst):
    """onepass_mul_kernel<A, KSH, MULTI, PTRS> (ntt_kernels_launch.h, launch_fwd_mul_impl: ma.one_pass -> launch_onepass_mul;
    host_ntt_domain.inc, fwd_mul: one_pass_pays, fwd_mul_ptrs_limb: ptrs_one_pass_mul): N = 2^15, NTT_OPT_ONE_PASS 1, the FP64
    policies; 5 polynomials on two workgroups per limb (onepass_grid: workgroup 0 takes polynomials 0, 2, 4, workgroup 1 takes
    1, 3); a is left as it was.  MULTI with PTRS is not built (launch_onepass_mul; fwd_mul_ptrs_limb hands a run over limb by
    limb).  Once per policy (slab): the store form with d_c = d_a and with d_c = d_bhat."""
    a = inst.args
    if a["MULTI"] and a["PTRS"]:
        return None
    nl = _nlimbs(a["MULTI"])
    opts = _grid_option((("OPT_ONE_PASS", 1),), 2, nl)
    out = _mul_forms(inst, a["KSH"], 15, nl, 5, opts, a["PTRS"], True)
    if nl == 1 and not a["PTRS"] and _first_class(inst):
        out += [_mul_case(inst, a["KSH"], 15, 1, 5, opts, alias=0, suffix="-alias-a"),
                _mul_case(inst, a["KSH"], 15, 1, 5, opts, alias=1, suffix="-alias-b")]
    return out


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
    "dot_inv_kernel": recipe_dot_inv,
    "fwd_mul_kernel": recipe_fwd_mul,
    "team_dot_kernel": recipe_team_dot,
    "team_mul_kernel": recipe_team_mul,
    "onepass_mul_kernel": recipe_onepass_mul,
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
    lib, oracle = rs.load()
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
