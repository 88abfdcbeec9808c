"""K3's two batched-load forms in the plan (alaz_amd/csrc/sg_plan.hpp: Plan::k3_in_form / k3_feat_lanes, Kernels likewise), on the CPU:
tests/micro/plan_driver.cpp, stage k3_forms, prints the plan's choice for a config line.

k3_in_form = 1: k3_in_part<1> issues every load of a trip before its first wait.  k3_feat_lanes = 1: the node-only feature launch runs
k3_node_features_lanes, eight lanes per node; it exists only where the score kernel computes the edge features (k5_efeat), because it
has no edge workgroups.  Unasked, the in-form follows k3_in_form_default (the shape of K5's form 1, where the A/B of
profiles/k3_forms_ab_c3.txt was run) and the lanes follow k5_efeat, each only while its constant (kK3InFormDefault,
kK3FeatLanesDefault) says the A/B passed the rule.  SG_K3_IN_FORM / SG_K3_FEAT_LANES name them in the development build; any value
but 0 and 1 is refused by name, and so is SG_K3_FEAT_LANES=1 beside k5_efeat = 0.  Neither moves the slices, the ranges or K5's plan."""
import pytest

from tests.plan_driver import run_named as run, stage_fixture
from tests.traces import C2, C3, C5_SHARD

SHAPES = [("c2", C2), ("c3", C3), ("c5_shard", C5_SHARD), ("c3_sharded", f"{C3} world=4 rank=1")]


exe = stage_fixture("k3_forms")


def test_the_defaults_per_configuration_line(exe):
    """C3 is the one shape that takes K5's form 1 and the inline edge features unasked: it alone can run the eight-lane kernel, and
    it alone was measured with k3_in_part<1>.  C2, a C5 shard and C3's graph sharded keep both at 0."""
    got = run(exe, [f"{n} {line}" for n, line in SHAPES])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k3_in_form"] == r["kernel_in_form"] and r["k3_feat_lanes"] == r["kernel_feat_lanes"], (n, r)
        assert r["k3_in_form"] == r["in_form_default"] == (r["in_form_on"] if n == "c3" else 0), (n, r)
        assert r["k3_feat_lanes"] == (r["feat_lanes_on"] if r["k5_efeat"] else 0), (n, r)
    assert [got[n]["k5_efeat"] for n, _ in SHAPES] == [1 if n == "c3" else 0 for n, _ in SHAPES]
    assert all(got[n]["k3_in_form"] == 0 and got[n]["k3_feat_lanes"] == 0 for n in ("c2", "c5_shard", "c3_sharded"))


def test_the_lanes_follow_the_inline_edge_features(exe):
    """asked for by name, K5's form 1 brings k5_efeat and with it the eight lanes; form 0 and SG_K5_EFEAT=0 take them away"""
    got = run(exe, [f"{n}_f1 {line} SG_K5_FORM=1" for n, line in SHAPES] + [f"c3_f0 {C3} SG_K5_FORM=0", f"c3_e0 {C3} SG_K5_EFEAT=0"])
    for n, _ in SHAPES:
        r = got[f"{n}_f1"]
        assert r["rc"] == 0 and r["k5_efeat"] == 1 and r["k3_feat_lanes"] == r["kernel_feat_lanes"] == r["feat_lanes_on"], (n, r)
    for n in ("c3_f0", "c3_e0"):
        assert got[n]["rc"] == 0 and got[n]["k5_efeat"] == 0 and got[n]["k3_feat_lanes"] == got[n]["kernel_feat_lanes"] == 0, got[n]
    assert got["c3_f0"]["k3_in_form"] == got["c3_e0"]["k3_in_form"] == got["c3_f0"]["in_form_default"]   # (the scan's form hangs on the shape, not on K5's knobs)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("lanes", [0, 1])
def test_the_overrides_in_every_combination(exe, form, lanes):
    got = run(exe, [f"c3 {C3} SG_K3_IN_FORM={form} SG_K3_FEAT_LANES={lanes}"] +
              [f"{n}_f1 {line} SG_K5_FORM=1 SG_K3_IN_FORM={form} SG_K3_FEAT_LANES={lanes}" for n, line in SHAPES])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k3_in_form"] == r["kernel_in_form"] == form and r["k3_feat_lanes"] == r["kernel_feat_lanes"] == lanes, (n, r)


def test_the_scan_form_is_legal_on_every_shape_and_zero_lanes_beside_form_0(exe):
    got = run(exe, [f"{n}_{f} {line} SG_K3_IN_FORM={f} SG_K3_FEAT_LANES=0" for n, line in SHAPES for f in (0, 1)])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k3_in_form"] == r["kernel_in_form"] == int(n[-1]) and r["k3_feat_lanes"] == r["kernel_feat_lanes"] == 0, (n, r)


BAD = ["2", "-1", "on", "", "01"]


@pytest.mark.parametrize("line,knob",
                         [(f"{C3} SG_K3_IN_FORM={v}", "SG_K3_IN_FORM") for v in BAD] + [(f"{C3} SG_K3_FEAT_LANES={v}", "SG_K3_FEAT_LANES") for v in BAD] +
                         [(f"{C3} SG_K5_EFEAT=0 SG_K3_FEAT_LANES=1", "SG_K3_FEAT_LANES"), (f"{C3} SG_K5_FORM=0 SG_K3_FEAT_LANES=1", "SG_K3_FEAT_LANES"),
                          (f"{C2} SG_K3_FEAT_LANES=1", "SG_K3_FEAT_LANES"), (f"{C5_SHARD} SG_K3_FEAT_LANES=1", "SG_K3_FEAT_LANES"),
                          (f"{C3} world=4 rank=1 SG_K3_FEAT_LANES=1", "SG_K3_FEAT_LANES")])
def test_refused_values(exe, line, knob):
    """anything but 0 and 1 — an A/B that silently ran one kernel twice would look like a tie —, and the eight lanes where
    k3_node_features has edge workgroups to run, by name or by default: the eight-lane kernel has none"""
    got = run(exe, [f"x {line}"])
    assert got["x"]["rc"] == -22 and knob in got["x"]["why"], got


def test_nothing_else_in_the_plan_moves(exe):
    got = run(exe, [f"c3_{f}{l} {C3} SG_K3_IN_FORM={f} SG_K3_FEAT_LANES={l}" for f in (0, 1) for l in (0, 1)] + [f"c3 {C3}"])
    for r in got.values():
        assert (r["k3_slices"], r["k3_ranges"], r["k5_form"], r["k5_efeat"]) == (48, 5, 1, 1), r   # what tests/golden/plans.json records for C3


def test_the_knobs_are_the_development_builds():
    from alaz_amd import engine
    assert "SG_K3_IN_FORM" in engine.DEV_KNOBS and "SG_K3_FEAT_LANES" in engine.DEV_KNOBS
