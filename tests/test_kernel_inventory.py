"""CPU: the static inventory of shipped kernel instances (tests/kernel_inventory.py) against the recipe table
(tests/kernel_recipes.py).  Reads the built gfx950 code objects; no GPU needed."""
import collections

import pytest

import kernel_inventory
import kernel_recipes


@pytest.fixture(scope="module")
def inventory():
    return kernel_inventory.instances()


def test_every_instance_parses_into_a_known_family(inventory):
    assert len(inventory) > 1000, "the inventory found only %d kernels: is the library built?" % len(inventory)
    unknown = sorted(k for k, i in inventory.items() if i.family is None)
    assert not unknown, "kernel instances of no known family (classify them in kernel_inventory.FAMILIES): %s" % unknown[:20]
    # the headline kernel is there, by name
    assert "fused_kernel<ArithF64,14,false,0,false,false,false>" in inventory


def test_every_instance_is_claimed_by_exactly_one_recipe_or_allowlisted(inventory):
    """every shipped instance: claimed by exactly one recipe, or allowlisted with a reason, or pinned in the list of instances
    not covered yet (tests/golden/uncovered_kernel_instances.txt) -- exactly one of the three"""
    pinned = kernel_recipes.uncovered()
    lost, twice, several = [], [], []
    for key, inst in sorted(inventory.items()):
        c = kernel_recipes.claims(inst)
        where = (len(c) > 0) + (key in kernel_recipes.ALLOWLIST) + (key in pinned)
        if where == 0:
            lost.append(key)
        elif len(c) > 1:
            twice.append((key, c))
        elif where > 1:
            several.append(key)
    assert not lost, ("instances no recipe claims (add a recipe, or an ALLOWLIST entry naming the dispatch line that rules them "
                      "out): %s" % lost)
    assert not twice, "instances claimed by several recipes: %s" % twice
    assert not several, "instances claimed and also allowlisted or pinned as not covered (drop the stale entry): %s" % several


def test_uncovered_list_names_shipped_instances_only(inventory):
    stale = sorted(kernel_recipes.uncovered() - set(inventory))
    assert not stale, "%s names instances the library no longer ships: %s" % (kernel_recipes.UNCOVERED_LIST, stale)


def test_allowlist_names_shipped_instances_with_reasons(inventory):
    for key, reason in kernel_recipes.ALLOWLIST.items():
        assert key in inventory, "stale allowlist entry: %s" % key
        assert isinstance(reason, str) and len(reason) > 20, "allowlist entry without a reason: %s" % key


def test_case_ids_are_unique(inventory):
    ids = collections.Counter(c.id for c in kernel_recipes.cases(inventory))
    assert not [i for i, n in ids.items() if n > 1]


@pytest.mark.parametrize("demangled,key", [
    ("void ntt::fused_kernel<ntt::ArithF64, 14, false, 0, false, false, false>(ntt::KArgs<ntt::ArithF64>)",
     "fused_kernel<ArithF64,14,false,0,false,false,false>"),
    ("void ntt::team_kernel<ntt::ArithU64X<3>, 5, true, 3, true>(ntt::KTeam<ntt::ArithU64X<3> >)",
     "team_kernel<ArithU64X<3>,5,true,3,true>"),
    ("void ntt::onepass_kernel<ntt::WideF64<ntt::ArithF64>, true, 0, false>(ntt::KArgs<ntt::WideF64<ntt::ArithF64>>)",
     "onepass_kernel<ArithF64W,true,0,false>"),
    ("ntt::team_ctl_clear_kernel(unsigned int*, unsigned long)", "team_ctl_clear_kernel"),
])
def test_names_normalise_as_a_kernel_trace_reports_them(demangled, key):
    """the object's demangled names and a trace's (`> >` or `>>`, with or without the return type) map to one key"""
    assert kernel_inventory.normalise(demangled) == key
    assert kernel_inventory.parse(key).family is not None
