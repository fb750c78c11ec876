"""GPU: every kernel instance the recipe table covers (tests/kernel_recipes.py) -- the transform families (onepass, twophase, team,
column), the coefficient-domain product families (fused_product, fused_product_small, team_product), the NTT-domain product
families (dot_inv, fwd_mul, team_dot, team_mul, onepass_mul) and the pointwise kernels -- launched and checked word for word
against the oracle; a kernel trace, one traced child per family, proves that the recipes launch every instance they claim; route
precedence of explicit plan options over the automatic one-pass choice."""
import os

import pytest

import children
import kernel_inventory
import kernel_recipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES_PY = os.path.join(ROOT, "tests", "kernel_recipes.py")

_CASES = kernel_recipes.cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_instance(lib, oracle, case):
    case.run(lib, oracle)


# Limit of each family's traced child, seconds: 3 x the untraced wall time of `python3 tests/kernel_recipes.py --family NAME` on an
# MI355X (in the comments), rounded up to a minute, at least 120 s.  A guard against a hang, not a performance claim.
FAMILY_LIMITS = {
    "onepass_kernel": 120,               # 1.7 s
    "twophase_kernel": 120,              # 1.9 s
    "team_kernel": 120,                  # 14.9 s
    "column_kernel": 120,                # 6.0 s
    "fused_product_kernel": 120,         # 4.3 s
    "fused_product_small_kernel": 120,   # 3.1 s
    "team_product_kernel": 120,          # 24.8 s
    "dot_inv_kernel": 120,               # 17.9 s
    "fwd_mul_kernel": 120,               # 13.5 s
    "team_dot_kernel": 180,              # 58.2 s
    "team_mul_kernel": 120,              # 29.4 s
    "onepass_mul_kernel": 120,           # 2.1 s
    "pointwise_kernel": 120,             # 1.0 s
    "pointwise_acc_kernel": 120,         # 0.8 s
    "pointwise_ptrs_kernel": 120,        # 0.8 s
}


_TRACES = {}   # family -> the kernels its traced child launched (one child per family and session)


def _family_trace(family):
    """(after a child that did not end cleanly, tests/children.py starts no further one)"""
    if family not in _TRACES:
        _TRACES[family] = set(children.traced(RECIPES_PY, ["--family", family], FAMILY_LIMITS[family]))
    return _TRACES[family]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(kernel_recipes.RECIPES))
def test_family_launches_the_instances_it_claims(family):
    """the traced child of one family launches every shipped instance of that family that is neither pinned as not covered nor
    allowlisted (the children run one per test, so that fifteen of them do not sit in one test without a sign of life)"""
    inv = kernel_inventory.instances()
    claimed = {k for k, i in inv.items() if i.family == family} - kernel_recipes.uncovered() - set(kernel_recipes.ALLOWLIST)
    missing = sorted(claimed - _family_trace(family))
    assert not missing, "instances the recipe names but never launches: %s" % missing


@pytest.mark.gpu
def test_every_covered_instance_is_launched():
    """the instances the recipes claim (every shipped instance outside tests/golden/uncovered_kernel_instances.txt) - launched -
    allowlist = {}, and no allowlisted instance is launched.  One traced child per family, one after the other (shared with the
    per-family test above; after a child that did not end cleanly no further one is started); the union of their traces is what
    is asserted."""
    inv = kernel_inventory.instances()
    assert set(FAMILY_LIMITS) == set(kernel_recipes.RECIPES)
    launched = set()
    for family in kernel_recipes.RECIPES:
        launched |= _family_trace(family)
    # the trace's names normalise to the inventory's: the headline kernel (the block pass behind the recipes' 1-stage column
    # passes) by name
    assert "fused_kernel<ArithF64,14,false,0,false,false,false>" in inv
    assert "fused_kernel<ArithF64,14,false,0,false,false,false>" in launched
    covered = set(inv) - kernel_recipes.uncovered()
    missing = sorted(covered - launched - set(kernel_recipes.ALLOWLIST))
    assert not missing, "instances the recipes name but never launch: %s" % missing
    stale = sorted(set(kernel_recipes.ALLOWLIST) & launched)
    assert not stale, "allowlisted instances that were launched: %s" % stale


@pytest.mark.gpu
@pytest.mark.parametrize("route,want,unwanted", [
    ("transform", "team_kernel", "onepass_kernel"),
    ("fwd_mul", "team_mul_kernel", "onepass_mul_kernel"),
])
def test_explicit_xcd_local_wins_over_the_automatic_one_pass_choice(route, want, unwanted):
    """N = 2^15, 50-bit prime, NTT_OPT_XCD_LOCAL 1, 131 polynomials (2 x 131 >= the CU count: the automatic one-pass choice
    would take it): the trace shows the XCD-local kernel and no one-pass kernel"""
    fams = {kernel_inventory.parse(k).family for k in children.traced(RECIPES_PY, ["--precedence", route], 300)}
    assert want in fams, (route, sorted(f for f in fams if f))
    assert unwanted not in fams, (route, sorted(f for f in fams if f))
