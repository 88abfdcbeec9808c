"""Where the edge features are computed, in the plan (alaz_amd/csrc/sg_plan.hpp: Plan::k5_efeat, Kernels::k5_efeat), on the CPU:
tests/micro/plan_driver.cpp, stage k5_efeat, prints the plan's choice for a config line.

k5_efeat = 1: k5_edge_score_lanes computes e_uv, lat_z and err_ratio of its own edge, k3_node_features launches no edge workgroups
and the engine holds no feature arrays.  It exists for form 1 only.  Unasked, an engine of form 1 takes it when kK5EfeatDefault says
so (the A/B of profiles/k5_efeat_ab_c3.txt) and an engine of form 0 never; SG_K5_EFEAT=0/1 names it in the development build, any
other value is refused, and so is 1 beside form 0.  k5_grid does not depend on it."""
import pytest

from tests.plan_driver import run_named as run, stage_fixture
from tests.traces import C2, C3, C5_SHARD

SHAPES = [("c2", C2), ("c3", C3), ("c5_shard", C5_SHARD), ("c3_sharded", f"{C3} world=4 rank=1")]


exe = stage_fixture("k5_efeat")


def test_the_default_follows_the_form(exe):
    """C3 is the one shape whose plan takes form 1 unasked: it alone can have the features inline.  C2, a C5 shard and C3's graph sharded
    keep form 0 and k3_node_features' edge workgroups."""
    got = run(exe, [f"{n} {line}" for n, line in SHAPES])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k5_efeat"] == r["kernel_efeat"], (n, r)
        assert r["k5_efeat"] == (r["efeat_default"] if r["k5_form"] == 1 else 0), (n, r)
    assert [got[n]["k5_form"] for n, _ in SHAPES] == [1 if n == "c3" else 0 for n, _ in SHAPES]
    assert all(got[n]["k5_efeat"] == 0 for n in ("c2", "c5_shard", "c3_sharded"))


def test_a_form_asked_for_by_name_takes_the_default_of_that_form(exe):
    got = run(exe, [f"{n}_{form} {line} SG_K5_FORM={form}" for n, line in SHAPES for form in (0, 1)])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k5_efeat"] == r["kernel_efeat"] == (r["efeat_default"] if n.endswith("_1") else 0), (n, r)


@pytest.mark.parametrize("efeat", [0, 1])
def test_the_override_in_both_directions(exe, efeat):
    got = run(exe, [f"c3 {C3} SG_K5_EFEAT={efeat}"] + [f"{n}_f1 {line} SG_K5_FORM=1 SG_K5_EFEAT={efeat}" for n, line in SHAPES])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k5_form"] == 1 and r["k5_efeat"] == r["kernel_efeat"] == efeat, (n, r)


def test_zero_is_legal_beside_form_0(exe):
    got = run(exe, [f"a {C2} SG_K5_EFEAT=0", f"b {C3} SG_K5_FORM=0 SG_K5_EFEAT=0"])
    assert all(r["rc"] == 0 and r["k5_form"] == 0 and r["k5_efeat"] == 0 for r in got.values()), got


@pytest.mark.parametrize("line", [f"{C3} SG_K5_EFEAT=2", f"{C3} SG_K5_EFEAT=-1", f"{C3} SG_K5_EFEAT=on", f"{C3} SG_K5_EFEAT=", f"{C3} SG_K5_EFEAT=01",
                                  f"{C3} SG_K5_FORM=0 SG_K5_EFEAT=1", f"{C2} SG_K5_EFEAT=1", f"{C5_SHARD} SG_K5_EFEAT=1", f"{C3} world=4 rank=1 SG_K5_EFEAT=1"])
def test_refused_values(exe, line):
    """anything but 0 and 1 — an A/B that silently ran one kernel twice would look like a tie —, and 1 where the form is 0, by name or
    by default: form 0 has no such kernel"""
    got = run(exe, [f"x {line}"])
    assert got["x"]["rc"] == -22 and "SG_K5_EFEAT" in got["x"]["why"], got


def test_k5_grid_does_not_depend_on_it(exe):
    got = run(exe, [f"c3_{e} {C3} SG_K5_EFEAT={e}" for e in (0, 1)] + [f"c2_{e} {C2} SG_K5_FORM=1 SG_K5_EFEAT={e}" for e in (0, 1)] + [f"c3 {C3}", f"c2 {C2}"])
    assert got["c3_0"]["k5_grid"] == got["c3_1"]["k5_grid"] == got["c3"]["k5_grid"] == 768           # what tests/golden/plans.json records
    assert got["c2_0"]["k5_grid"] == got["c2_1"]["k5_grid"] == -(-66596 // 256) and got["c2"]["k5_grid"] == 768


def test_the_knob_is_the_development_builds():
    from alaz_amd import engine
    assert "SG_K5_EFEAT" in engine.DEV_KNOBS
