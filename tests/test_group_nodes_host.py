"""CPU tests of the workload rows (K16): the two references of tests/group_nodes_ref.py held together (numpy over the group edges;
plain Python over the window's rows), against the node rollup's reference where the map groups nothing, the ordering claim the
baseline's merge rests on (ascending group key is strictly ascending workload key), the baseline reference against a hand-computed
rollout, the selection reference, and the plans in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage group_nodes)."""
import json
import os

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.group_nodes_ref import (GroupNodeTrendRef, gk_of_refs, group_nodes_ref, group_nodes_rows, ref_select_group_nodes)
from tests.group_ref import group_ref
from tests.group_trend_ref import workload_keys
from tests.helpers import ref
from tests.node_trend_ref import NodeTrendRef
from tests.nodes_ref import NO_ROW, nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests.traces import _random_map, _random_rows
from tests.trend_ref import REF_KNOWN, REF_LABEL, REF_OBIP

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP
NOOB = np.zeros(0, np.uint32)


def G(g):
    return ref(engine.REF_GROUP, g)


def rows_of(*edges):
    """canonical-order rows from (from_ref, to_ref, count, err_count, sum_ns[, score[, alive]]) tuples (sorted here)"""
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, e in enumerate(sorted(edges)):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["count"], r[i]["err_count"], r[i]["sum_ns"] = e[:5]
        if len(e) > 5:
            r[i]["score"] = e[5]
        if len(e) > 6:
            r[i]["alive"] = e[6]
    return r


# ---- the two references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_the_group_edge_and_the_row_formulations_agree(seed):
    """random windows with self-loops, alive-only rows, NaN, ties in score, -0.0 and +0.0 (tests/test_group_host._random_rows)"""
    rng = np.random.default_rng(1600 + seed)
    mk, ml = int(rng.integers(41, 200)), int(rng.integers(1, 30))     # (_random_rows' sources are KNOWN ids below max(mk, ml, 40))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 6 * mk)))
    mg = int(rng.integers(1, mk + 1))
    inside = 0
    for gmap in (_random_map(rng, mk, mg), _random_map(rng, mk, mg, 1.0, block=7), np.zeros(mk, np.uint32), np.full(mk, NO, np.uint32)):
        ge, _, _ = group_ref(rows, gmap, mg, mk, ml)
        a, b = group_nodes_ref(ge, mg, mk, ml), group_nodes_rows(rows, gmap, mg, mk, ml)
        assert a.dtype == b.dtype == engine.NODE_DTYPE and a.tobytes() == b.tobytes()
        k = gk_of_refs(a["ref"], mg, mk, ml)
        assert (k[1:] > k[:-1]).all()                                  # one row per node, ascending by group key
        assert int(a["out_edges"].sum()) == int(a["in_edges"].sum()) == len(ge)
        inside += int((ge["from_ref"] == ge["to_ref"]).sum())
        for f in ("count", "err", "sum_ns", "sumsq_us", "score_q32"):  # every group edge once on each side (wrapping sums)
            src = {"count": "count", "err": "err_count"}.get(f, f)
            with np.errstate(over="ignore"):
                tot = np.add.reduce(ge[src].astype(np.uint64))
                assert np.add.reduce(a[f"out_{f}"]) == tot == np.add.reduce(a[f"in_{f}"])
    if ((rows["to_ref"] >> 30) == REF_KNOWN).any():                   # (the map of zeros puts every KNOWN node into workload 0)
        assert inside > 0                                             # group edges inside a workload: on both sides of its row


def test_fields_by_hand():
    """workload 3 = pods 0, 1; pod 2 ungrouped; label 0.  Rows: 0->2, 1->2 (one group edge 3->2), 0->1 (inside workload 3), 2->label"""
    a, b, c, lab = ref(REF_KNOWN, 0), ref(REF_KNOWN, 1), ref(REF_KNOWN, 2), ref(REF_LABEL, 0)
    rows = rows_of((a, c, 2, 1, 100, 0.5, 1), (b, c, 3, 0, 200, 0.5, 2), (a, b, 7, 2, 70, -0.0, 0), (c, lab, 0, 0, 0, 0.0, 5))
    gmap = np.array([3, 3, NO, NO], np.uint32)
    for n in (group_nodes_rows(rows, gmap, 8, 4, 2), group_nodes_ref(group_ref(rows, gmap, 8, 4, 2)[0], 8, 4, 2)):
        assert n["ref"].tolist() == [G(3), c, lab]                    # the group first: not the order of the raw ref words
        assert n["ref"].tolist() != sorted(n["ref"].tolist())
        w = n[0]                                                      # rows in canonical order: (a, b) 0, (a, c) 1, (b, c) 2, (c, lab) 3
        assert (w["out_edges"], w["out_count"], w["out_err"], w["out_sum_ns"], w["out_alive"]) == (2, 12, 3, 370, 3)
        assert (w["in_edges"], w["in_count"], w["in_err"], w["in_sum_ns"], w["in_alive"]) == (1, 7, 2, 70, 0)   # the inside edge
        assert w["out_score_max"] == np.float32(0.5) and w["out_worst_row"] == 1   # the smallest row among the equal scores
        assert w["in_worst_row"] == 0 and w["in_score_max"].tobytes() == np.float32(-0.0).tobytes()
        assert w["score"] == np.float32(0.5) and w["out_score_q32"] == 1 << 32
        p = n[1]
        assert (p["in_edges"], p["in_count"], p["out_edges"], p["out_count"], p["out_alive"]) == (1, 5, 1, 0, 5)
        assert p["out_worst_row"] == 3 and p["out_score_max"].tobytes() == np.float32(0.0).tobytes()
        assert n[2]["out_edges"] == 0 and n[2]["out_worst_row"] == NO_ROW and n[2]["out_score_max"] == 0 and n[2]["in_alive"] == 5


@pytest.mark.parametrize("seed", range(4))
def test_a_map_that_groups_nothing_gives_the_node_rollup(seed):
    rng = np.random.default_rng(1700 + seed)
    mk, ml = int(rng.integers(41, 120)), int(rng.integers(1, 20))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 5 * mk)))
    gmap = np.full(mk, NO, np.uint32)
    ge, _, _ = group_ref(rows, gmap, 9, mk, ml)
    want = nodes_ref(rows)
    assert group_nodes_ref(ge, 9, mk, ml).tobytes() == want.tobytes() == group_nodes_rows(rows, gmap, 9, mk, ml).tobytes()


def test_an_empty_window():
    assert len(group_nodes_ref(np.zeros(0, engine.GROUP_EDGE_DTYPE), 4, 4, 4)) == 0
    assert len(group_nodes_rows(np.zeros(0, EDGE_OUT_DTYPE), np.zeros(4, np.uint32), 4, 4, 4)) == 0


# ---- the ordering claim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_ascending_group_key_is_strictly_ascending_workload_key(seed):
    """across groups, KNOWN, LABEL and OBIP: the outbound-IP list is ascending, so OBIP indices ascend as their addresses do"""
    rng = np.random.default_rng(1800 + seed)
    mg, mk, ml, mob = int(rng.integers(1, 50)), int(rng.integers(1, 50)), int(rng.integers(1, 20)), int(rng.integers(1, 40))
    obips = np.sort(rng.choice(np.arange(1, 1 << 32, 65537, dtype=np.uint64), mob, replace=False)).astype(np.uint32)
    refs = np.array([G(g) for g in range(mg)] + [ref(REF_KNOWN, v) for v in range(mk)] + [ref(REF_LABEL, v) for v in range(ml)]
                    + [ref(REF_OBIP, v) for v in range(mob)], np.uint32)
    gk = gk_of_refs(refs, mg, mk, ml)
    assert gk.tolist() == list(range(mg + mk + ml + mob))
    pick = np.sort(rng.choice(len(refs), int(rng.integers(1, len(refs) + 1)), replace=False))
    wk = workload_keys(refs[pick], obips)
    assert (wk[1:] > wk[:-1]).all()
    assert wk[0] == (pick[0] if pick[0] < mg else wk[0]) and (wk[pick < mg] == pick[pick < mg]).all()   # a group's key is its id
    rows = _random_rows(rng, mk + 41, ml, 200)
    gmap = _random_map(rng, mk + 41, mg)
    n = group_nodes_ref(group_ref(rows, gmap, mg, mk + 41, ml)[0], mg, mk + 41, ml)
    ob40 = np.sort(rng.choice(np.arange(1, 1 << 32, 65537, dtype=np.uint64), 40, replace=False)).astype(np.uint32)
    wk = workload_keys(n["ref"], ob40)
    assert (wk[1:] > wk[:-1]).all()
    GroupNodeTrendRef(len(n)).window(n, ob40)                          # (the reference asserts it of its 2 N samples too)


# ---- the baseline ------------------------------------------------------------------------------------------------------------------
def _entry(t, fk, side):
    e = t.entries[(t.entries["from_key"] == fk) & (t.entries["to_key"] == side)]
    return e[0] if len(e) else None


def test_a_rollout_keeps_the_workloads_entry_and_resets_the_pods():
    """workload 0 = pods 0..7 calls service node 20.  Pods 0..3 carry the traffic for warmup + 2 windows, then pods 4..7 (new pods,
    new ids) with the latency stepped up: K10's pod rows are new nodes, the workload's out side goes on counting — by hand"""
    warmup, mk, ml = 2, 24, 4
    gmap = np.full(mk, NO, np.uint32); gmap[:8] = 0
    svc = ref(REF_KNOWN, 20)
    pod, wl = NodeTrendRef(mk + ml, shift=1, warmup=warmup), GroupNodeTrendRef(mk + ml, shift=1, warmup=warmup)
    pv, gv, gn = [], [], None
    for w in range(warmup + 4):
        half = range(0, 4) if w < warmup + 2 else range(4, 8)
        lat = 1000 if w < warmup + 2 else 5000
        rows = rows_of(*[(ref(REF_KNOWN, p), svc, 2, 0, 2 * lat) for p in half])
        gn = group_nodes_rows(rows, gmap, 8, mk, ml)
        assert gn["ref"].tolist() == [G(0), svc] and gn["out_count"][0] == 8 and gn["in_count"][1] == 8 and gn["out_edges"][0] == 1
        pv.append(pod.window(nodes_ref(rows), NOOB)); gv.append(wl.window(gn, NOOB))
    sw = warmup + 2
    assert (pv[sw]["out_seen"][:4] == 0).all() and (pv[sw]["out_lat_dev"][:4] == 0).all()   # four new pods
    assert pv[sw]["in_seen"][4] == sw                                  # the service node is the same node
    assert gv[sw]["out_seen"][0] == sw and gv[sw]["out_lat_dev"][0] == np.float32(4000 / 1000) and gv[sw]["out_base_mean_us"][0] == np.float32(1.0)
    assert gv[sw]["in_seen"][0] == 0 and gv[sw]["in_lat_dev"][0] == 0  # workload 0 receives nothing: no entry on its in side
    assert gv[sw]["in_seen"][1] == sw and gv[sw + 1]["out_seen"][0] == sw + 1 and gv[sw + 1]["in_seen"][1] == sw + 1
    assert [(int(e["from_key"]), int(e["to_key"])) for e in wl.entries] == [(0, 1), ((1 << 32) | 20, 0)]   # (wk, side)
    e = _entry(wl, 0, 1)
    assert e["n"] == warmup + 4 and e["last"] == warmup + 4
    # x = 1000 four times, then 5000 twice with alpha = 1/2: mean 1000 -> 3000 -> 4000
    assert e["lat_mean"] == 4000.0
    assert len(pod.entries) == 9                                      # eight pods' out sides and the service's in side


def test_a_side_without_requests_neither_creates_nor_refreshes():
    t = GroupNodeTrendRef(16, shift=1, warmup=1, ttl=2)
    a, b = ref(REF_KNOWN, 0), ref(REF_KNOWN, 1)
    gmap = np.array([2, NO], np.uint32)
    alive = group_nodes_rows(rows_of((a, b, 0, 0, 0, 0.0, 3)), gmap, 4, 2, 1)
    t.window(alive, NOOB)
    assert len(t.entries) == 0
    t.window(group_nodes_rows(rows_of((a, b, 2, 0, 200)), gmap, 4, 2, 1), NOOB)
    assert [(int(e["from_key"]), int(e["to_key"]), int(e["last"])) for e in t.entries] == [(2, 1, 2), ((1 << 32) | 1, 0, 2)]
    o = t.window(alive, NOOB)                                          # reported, not refreshed
    assert o["out_seen"].tolist() == [1, 0] and o["in_seen"].tolist() == [0, 1] and _entry(t, 2, 1)["last"] == 2
    t.window(alive, NOOB)
    assert len(t.entries) == 0 and t.stats["expired"] == 2


def test_default_capacity_is_four_times_the_row_capacity():
    assert GroupNodeTrendRef(100).cap == 400 and GroupNodeTrendRef(100, max_entries=7).cap == 7


# ---- the selection -----------------------------------------------------------------------------------------------------------------
def test_selection_reference():
    n = np.zeros(6, engine.NODE_DTYPE)
    n["score"] = np.array([0.5, 0.9, -0.0, 0.9, np.nan, 0.0], np.float32)
    n["in_count"] = [1, 0, 0, 2, 0, 0]; n["out_count"] = [0, 0, 3, 0, 0, 0]
    tr = np.zeros(6, engine.NODE_TREND_DTYPE)
    tr["out_lat_dev"] = [1.0, 3.0, 2.0, 3.0, 0.0, np.nan]
    tr["in_seen"] = [0, 0, 0, 4, 0, 0]
    assert list(ref_select_group_nodes(n, None, "score", 0, 0.0)) == [0, 1, 2, 3, 5]      # NaN never, -0.0 >= 0.0
    assert list(ref_select_group_nodes(n, None, "score", 3, float("-inf"))) == [1, 3, 0]  # ties by position
    assert list(ref_select_group_nodes(n, tr, "out_lat_dev", 2, 0.0)) == [1, 3]
    assert list(ref_select_group_nodes(n, tr, "out_lat_dev", 0, 2.0)) == [1, 2, 3]
    assert list(ref_select_group_nodes(n, tr, "new", 0, 99.0)) == [0, 2]                  # requests on a side, nothing seen on either
    assert list(ref_select_group_nodes(n, tr, "new", 1, 0.0)) == [0]


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("group_nodes")


def _p(me, ncap, mg, slots=1, maxe=0, cb=512):
    return (me, ncap, mg, slots, maxe, cb)


def _slices(me, gk):
    ranges = -(-gk // 2048)
    return min(16, -(-max(me, 1) // 32768), max(1, 1024 // ranges))


CASES = [_p(me, ncap, mg, slots) for me in (0, 1, 2047, 2048, 4097, 1 << 15, 1 << 16, 1_250_000, 1 << 24)
         for ncap, mg in ((1, 1), (500, 10), (2000, 48), (2000, 49), (41280, 65536), (1 << 20, 1 << 20), (3, (1 << 21) - 3))
         for slots in (1, 3)]


def test_plan_layout_for_every_case(plan):
    for r in plan(CASES):
        me, gk = max(r["max_edges"], 1), r["ncap"] + r["max_groups"]
        assert r["rc"] == 0 and r["node_size"] == 136 and r["node_trend_size"] == 32 and r["gk"] == gk
        nc = r["nc"]
        assert nc == min(gk, 2 * me) and r["out_wgs"] == -(-me // 2048) and r["ranges"] == -(-gk // 2048)
        assert r["slices"] == _slices(me, gk) and 1 <= r["ranges"] * r["slices"] <= max(1024, r["ranges"])
        assert r["node_per"] % 256 == 0 and 1 <= r["node_wgs"] <= r["max_wgs"] == 1024 and r["node_wgs"] * r["node_per"] >= gk
        assert (r["node_wgs"] - 1) * r["node_per"] < gk                # no workgroup without a key in front of one with keys
        assert r["lds_bytes"] == 2048 * 64 <= r["lds_limit"]
        need = {"table_out": 64 * gk, "table_in": 64 * gk, "part": 64 * 2048 * r["ranges"] * r["slices"], "dst": 4 * me, "blk": 2 * 1024 * 4,
                "rows": 136 * nc, "count": 8}
        check_layout(r, need, per_slot=("rows", "count"))
        t = r["trend"]                                                # two samples per row; max_entries 0 = 4 x the row capacity
        assert t["rc"] == 0 and t["entries"] == t["max_entries"] == min(1 << 31, 4 * nc) and 1 <= t["wgs"] <= 1024
        if t["wgs"] < 1024:
            assert t["wgs"] * 256 * t["per_thread"] >= t["entries"] + 2 * nc
        check_layout(t, {"soa0": 56 * t["entries"], "soa1": 56 * t["entries"], "ctl": 64, "blk": 16 * t["wgs"], "thread": 16 * 256 * t["wgs"],
                         "rows": 32 * nc}, per_slot=("rows",))
        check_soa(t)
        s = r["sel"]                                                  # K7's scratch over NC keys, NC indices, NC rows of staging
        assert s["key_bytes"] == 4 * nc and 1 <= s["wgs"] <= 1024 and (s["wgs"] == 1024 or s["wgs"] * 2048 >= nc)
        check_layout(s, {"stage": 136 * nc, "ctr": 512, "idx": 4 * nc, "sel": s["scratch_bytes"]})
        k7 = {"pairs": 8 * engine.SELECT_MAX_K, "state": 8 + 4 * 8, "blk": 16 * s["wgs"], "hist": 1024 * s["wgs"], "keys": 4 * nc}
        check_layout(s, k7, align=8, layout="k7_layout", total="scratch_bytes", tail_align=4)


def test_plan_refuses_more_than_two_to_the_21_keys(plan):
    r = plan([_p(1000, 1, (1 << 21) - 1), _p(1000, 1, 1 << 21), _p(1000, 1 << 21, 1), _p(1000, 1 << 20, (1 << 20) + 1),
              _p(1000, 0xFFFFFFFF, 0xFFFFFFFF)])
    assert [x["rc"] for x in r] == [0, engine.SG_EINVAL, engine.SG_EINVAL, engine.SG_EINVAL, engine.SG_EINVAL]
    top = r[0]
    assert top["gk"] == 1 << 21 and top["table_bytes"] == 128 << 20 and top["part_bytes"] == 128 << 20   # 256 MB of tables, 128 MB of partials


def test_plan_slices_rule(plan):
    a, b, c, d = plan([_p(1 << 24, 2047, 1), _p(1 << 24, 2048, 1), _p(1 << 24, (1 << 21) - 1, 1), _p(1 << 16, 2047, 1)])
    assert (a["gk"], a["ranges"], a["slices"]) == (2048, 1, 16)       # one range: the slices are the rows' alone
    assert (b["gk"], b["ranges"], b["slices"]) == (2049, 2, 16)
    assert (c["gk"], c["ranges"], c["slices"]) == (1 << 21, 1024, 1)  # many ranges take fewer slices
    assert d["slices"] == 2                                           # the GPU tests' engines: max_edges 65 536
    m, = plan([_p(1 << 24, 200_000, 4800)])
    assert m["ranges"] == 100 and m["slices"] == 10


def test_plan_trend_capacity_override_and_config_3(plan, capsys):
    k, = plan([_p(1000, 50, 50, maxe=7)])
    assert k["trend"]["entries"] == 7
    bad, = plan([_p(1000, 50, 50, maxe=(1 << 31) + 1)])
    assert bad["trend"]["rc"] == engine.SG_EINVAL
    c3, = plan([_p(1_250_000, 40_000 + 1024 + 256, 65536, 3)])       # config 3's max_edges, 40 k known nodes, 64 Ki groups, three window slots
    with capsys.disabled():
        print("\nconfig 3: " + json.dumps({f: c3[f] for f in ("gk", "nc", "out_wgs", "ranges", "slices", "node_wgs", "node_per", "total_bytes")}))
    assert c3["total_bytes"] < 256 << 20 and c3["ranges"] * c3["slices"] <= 1024


# ---- GraphDS: the switches forwarded, group ids resolved back to owner UIDs (the recording stand-in engine of host_capi.cpp) ----
def test_graphds_workload_rows_against_the_stand_in_engine():
    from alaz_amd import hostlib
    ds = hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")                  # node 1, workload 1 = sts-q
    assert ds.set_workload_nodes() == 0 and ds.set_workload_node_trend(shift=3, warmup=2, ttl=9) == 0 and ds.set_workload_node_trend() == 0
    n = ds.workload_nodes()
    assert n["row"].dtype == engine.NODE_DTYPE and n.dtype.itemsize == 16 + 160 + 136
    assert [(r["type"], r["uid"]) for r in n] == [(b"workload", b"sts-q"), (b"workload", b"dep-a"), (b"pod", b"pod-0")]
    assert n["row"]["out_count"].tolist() == [9, 4, 0] and n["row"]["in_edges"].tolist() == [0, 1, 1] and n["row"]["score"].tolist() == [0.75, 0.5, 0.25]
    assert n["row"]["ref"].tolist() == [G(1), G(0), 0] and (n["row"]["out_worst_row"] == NO_ROW).all()
    t = ds.workload_node_trends()
    assert t.dtype == engine.NODE_TREND_DTYPE and t["in_seen"].tolist() == [1, 2, 3] and t["out_lat_dev"].tolist() == [-0.25] * 3
    rows, idx = ds.workload_nodes_top(engine.NSEL_BY["in_lat_dev"], 5, 1.5)
    assert idx.tolist() == [2, 0] and [(r["type"], r["uid"]) for r in rows] == [(b"pod", b"pod-0"), (b"workload", b"sts-q")]
    assert rows["row"]["in_count"].tolist() == [4, 0]
    rows, idx = ds.workload_nodes_top(engine.NSEL_BY["score"], 0)     # k = 0: the count first, then the rows
    assert idx.tolist() == [2, 0] and len(rows) == 2
    ds.set_workload_nodes(False)
    bits = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])   # noqa: E731
    assert [tuple(int(x) for x in r) for r in ds.mock_k16_ops()] == \
        [(1, 1, 0, 0), (2, 3, 2, 9), (2, 0, 0, 0)] + [(3, 1, 5, bits(1.5))] * 2 + [(3, 0, 0, bits(float("-inf")))] * 4 + [(1, 0, 0, 0)]
