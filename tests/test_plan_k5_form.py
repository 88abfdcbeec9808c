"""k5_edge_score's form in the plan (alaz_amd/csrc/sg_plan.hpp: Plan::k5_form, Plan::k5_grid, Kernels::k5_form), on the CPU:
tests/micro/plan_driver.cpp, stage k5_form, prints the plan's choice for a config line.

Form 0 gives sixteen lanes to an edge (32 edges per workgroup and step, three workgroups per CU), form 1 one lane (256 edges per
workgroup and step; a CU holds as many of its workgroups as its LDS — 32 KiB each — and its registers — three waves per SIMD —
allow).  k5_grid is one round of the chosen form's workgroups, or fewer where max_edges needs fewer."""
import pytest

from tests.plan_driver import run_named as run, stage_fixture
from tests.traces import C2, C3, C5_SHARD

SHAPES = [("c2", C2), ("c3", C3), ("c5_shard", C5_SHARD)]


exe = stage_fixture("k5_form")


def grid(r, form):
    per_wg, per_cu = (256, min(r["lds_cap"] // r["lanes_wg_lds"], r["lanes_waves"])) if form else (32, 3)
    return max(1, min(-(-r["max_edges"] // per_wg), per_cu * r["cus"]))


def test_the_default_form_of_c2_c3_and_a_c5_shard(exe):
    """the plan takes form 1 only where it was measured to win (profiles/k5_lanes_ab_c3.txt): unsharded engines of 2^20 edges and
    more — C3; C2, a C5 shard and C3's graph sharded keep form 0"""
    got = run(exe, [f"{n} {line}" for n, line in SHAPES] + [f"c4 {C3} world=4 rank=1", f"below {C3.replace('1254096', '1048575')}", f"at {C3.replace('1254096', '1048576')}"])
    want = {"c2": 0, "c3": 1, "c5_shard": 0, "c4": 0, "below": 0, "at": 1}
    for n, form in want.items():
        r = got[n]
        assert r["rc"] == 0 and r["k5_form"] == r["kernel_form"] == r["form_default"] == form, (n, r)
        assert r["k5_grid"] == grid(r, form), (n, r)
    assert got["c3"]["lanes_min_edges"] == 1 << 20
    assert got["c3"]["k5_grid"] == 768 and got["c2"]["k5_grid"] == 768                         # what tests/golden/plans.json records: unchanged by the form


@pytest.mark.parametrize("form", [0, 1])
def test_the_override_wins_and_the_grid_is_the_forms_own(exe, form):
    got = run(exe, [f"{n} {line} SG_K5_FORM={form}" for n, line in SHAPES] + [f"small max_known_nodes=100 max_edges=1000 SG_K5_FORM={form}",
                                                                               f"half {C3} cus=128 SG_K5_FORM={form}"])
    for n, r in got.items():
        assert r["rc"] == 0 and r["k5_form"] == r["kernel_form"] == form, (n, r)
        assert r["k5_grid"] == grid(r, form), (n, r)
    assert got["c3"]["k5_grid"] == 768 and got["half"]["k5_grid"] == 384                       # three workgroups per CU in either form
    assert got["small"]["k5_grid"] == (4 if form else 32)
    assert got["c3"]["lanes_wg_lds"] * 3 <= got["c3"]["lds_cap"]


def test_sg_k5_grid_still_overrides_the_round(exe):
    got = run(exe, [f"a {C3} SG_K5_FORM=1 SG_K5_GRID=1024", f"b {C3} SG_K5_FORM=0 SG_K5_GRID=1024", f"c {C2} SG_K5_FORM=1 SG_K5_GRID=1024"])
    assert got["a"]["k5_grid"] == 1024 and got["b"]["k5_grid"] == 1024
    assert got["c"]["k5_grid"] == -(-66596 // 256)                                             # never more workgroups than batches of 256 edges


@pytest.mark.parametrize("value", ["2", "-1", "lanes", "", "01"])
def test_an_unknown_form_is_refused(exe, value):
    got = run(exe, [f"x {C3} SG_K5_FORM={value}"])
    assert got["x"]["rc"] == -22 and "SG_K5_FORM" in got["x"]["why"], got


def test_the_knob_is_the_development_builds():
    from alaz_amd import engine
    assert "SG_K5_FORM" in engine.DEV_KNOBS
