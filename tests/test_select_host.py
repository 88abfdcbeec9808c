"""CPU tests of the selection (K7) plumbing: GraphDS::SetSelection reaches the engine's sg_flush_window_top (through the recording
stand-in of alaz_amd/csrc/host/host_capi.cpp), and the selection's plan in alaz_amd/csrc/sg_plan.hpp sizes its scratch for every
window an engine can close (tests/micro/plan_driver.cpp, stage select)."""
import math
import os


from alaz_amd import engine, hostlib
from alaz_amd.engine import make_config
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout

HERE = os.path.dirname(os.path.abspath(__file__))


def _mock_graphds(max_edges=4096):
    return hostlib.GraphDS(make_config(max_known_nodes=64, max_edges=max_edges), engine_lib=None)


def test_set_selection_reaches_flush_window_top_with_k_and_min_score():
    g = _mock_graphds()
    try:
        assert g.set_selection(1000, 0.75) == 0
        g.PersistPod("pod-a", "10.0.0.1")
        n, rows = g.FlushWindowRows(1234)
        assert n == 0 and rows == []
        f = g.mock_flushes()
        assert f == {"flush_window": 0, "flush_window_top": 1, "k": 1000, "min_score": 0.75}
        assert g.set_selection(0, float("-inf")) == 0          # threshold mode
        g.FlushWindow()
        f = g.mock_flushes()
        assert f["flush_window_top"] == 2 and f["k"] == 0 and f["min_score"] == -math.inf
        assert g.set_selection(engine.SELECT_MAX_K + 1, 0.0) == engine.SG_EINVAL   # refused: the selection stays as it was
        g.FlushWindow()
        assert g.mock_flushes()["k"] == 0 and g.mock_flushes()["flush_window_top"] == 3
        g.clear_selection()
        g.FlushWindow()
        assert g.mock_flushes()["flush_window"] == 1 and g.mock_flushes()["flush_window_top"] == 3
    finally:
        g.close()


def test_graphds_without_a_selection_never_calls_flush_window_top():
    g = _mock_graphds()
    try:
        for _ in range(3):
            g.FlushWindow()
        f = g.mock_flushes()
        assert f["flush_window"] == 3 and f["flush_window_top"] == 0
    finally:
        g.close()


sel_plan = plan_fixture("select")


SIZES = [1, 2, 255, 2047, 2048, 2049, 4096, 1 << 15, 1 << 18, (1 << 20) - 1, 1 << 20, 2_000_000, 1 << 21, (1 << 21) + 1, 1 << 22, 1 << 24]


def test_select_scratch_covers_every_window(sel_plan):
    for r in sel_plan(SIZES):
        me, p = r["max_edges"], r["used"]
        assert 1 <= p["wgs"] <= r["max_wgs"] == 1024
        assert p["key_bytes"] >= 4 * me                          # one key per row
        assert p["hist_bytes"] == p["wgs"] * 256 * 4 and p["blk_bytes"] == p["wgs"] * 16
        assert p["pair_bytes"] >= 8 * r["max_k"]                 # the top-k's (key, index) pairs
        assert p["state_bytes"] >= 8 * 4 + 8
        assert p["scratch_bytes"] == sum(p[k] for k in ("key_bytes", "hist_bytes", "blk_bytes", "pair_bytes", "state_bytes"))
        assert p["stage_rows"] >= me                             # threshold mode may select every row
        k7 = {"pairs": 8 * r["max_k"], "state": 8 * 4 + 8, "blk": p["wgs"] * 16, "hist": p["wgs"] * 256 * 4, "keys": 4 * me}
        check_layout({**p, "layout": r["layout"]}, k7, align=8, total="scratch_bytes", slots=1, tail_align=4)
        # the rows are split into wgs contiguous spans: below the workgroup cap a span is at most rows_per_wg rows
        if me <= r["max_wgs"] * r["rows_per_wg"]:
            assert p["wgs"] * r["rows_per_wg"] >= me
    # BASELINE config 3: 1 M edges in 512 spans of 2048
    c3 = {r["max_edges"]: r["used"] for r in sel_plan([1 << 20])}[1 << 20]
    assert c3["wgs"] == 512


def test_node_selection_block(sel_plan):
    """plan_node_select over max_edges node rows: the row staging, the counter block, the index array, then K7's scratch at its offset"""
    for r in sel_plan(SIZES):
        nc, n = r["max_edges"], r["node"]
        assert n["sel_layout"] == r["layout"] and n["sel_scratch_bytes"] == r["used"]["scratch_bytes"]   # K7's plan over the node rows
        check_layout(n, {"stage": nc * 136, "ctr": n["ctr_in"], "idx": nc * 4, "sel": n["sel_scratch_bytes"]}, slots=1)
        assert [p[0] for p in n["layout"]] == ["stage", "ctr", "idx", "sel"] and n["layout"][3][1] == n["sel_off"]
        by = {p[0]: p[2] for p in n["layout"]}
        assert n["total_bytes"] == sum(by.values()) and by["sel"] - n["sel_scratch_bytes"] < 256      # what the engine allocated before the plan had it


def test_top_k_sort_fits_a_workgroups_lds(sel_plan):
    r = sel_plan([1 << 20])[0]
    assert r["max_k"] == engine.SELECT_MAX_K == 16384
    assert r["sort_lds_max_k"] == 16384 * 8 <= r["lds_bytes"] == 160 * 1024
    assert r["sort_lds_1"] == 8


def test_no_scratch_when_selection_is_never_used(sel_plan):
    for r in sel_plan(SIZES):
        assert all(v == 0 for v in r["unused"].values()), r["unused"]
