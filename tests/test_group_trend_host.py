"""CPU tests of the workload baselines (K15): the numpy reference tests/group_trend_ref.py against hand-computed sequences, the
ordering claim the merge rests on (a window's group edges are strictly ascending in their workload keys), the rollout sequence on
reference rows (the pod-level baseline forgets, the workload-level one does not), the plans in alaz_amd/csrc/sg_plan.hpp
(tests/micro/plan_driver.cpp, stage group_trend), and the front end's new methods against the recording stand-in of
tests/test_engine_front.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests.abi_layouts import LAYOUTS
from tests import engine_front as front
from tests.group_ref import group_ref
from tests.group_trend_ref import GroupTrendRef, GroupVanishRef, group_keys, ref_select_groups, workload_keys
from tests.helpers import ref
from tests.host_scaffold import node_trend_rows_of as rows_of
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests.traces import _random_map, _random_rows
from tests.trend_ref import REF_KNOWN, REF_LABEL, REF_OBIP, TrendRef, strictly_ascending
from tests.vanish_ref import NO_ROW

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP
NOOB = np.zeros(0, np.uint32)


def G(g):
    return ref(engine.REF_GROUP, g)


def edges_of(*edges):
    """group edges from (from_ref, to_ref, count, err_count, sum_ns) tuples, in the order given (the caller's: key order)"""
    r = np.zeros(len(edges), dtype=engine.GROUP_EDGE_DTYPE)
    for i, (f, t, c, e, s) in enumerate(edges):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["count"], r[i]["err_count"], r[i]["sum_ns"] = f, t, c, e, s
    return r


def _entry(t, fk, tk):
    e = t.entries[(t.entries["from_key"] == fk) & (t.entries["to_key"] == tk)]
    return e[0] if len(e) else None


# ---- the reference against hand-computed sequences ----------------------------------------------------------------------------
def test_workload_keys():
    obips = np.array([0x0A000001, 0xC0A80001], np.uint32)
    refs = [G(0), G(7), ref(REF_KNOWN, 7), ref(REF_LABEL, 3), ref(REF_OBIP, 1)]
    assert workload_keys(refs, obips).tolist() == [0, 7, (1 << 32) | 7, (2 << 32) | 3, (3 << 32) | 0xC0A80001]


def test_a_grouped_pair_across_three_windows():
    t = GroupTrendRef(64, shift=1, warmup=1)                          # alpha = 1/2
    o = t.window(edges_of((G(1), G(2), 2, 0, 2000)), NOOB)            # x_lat = 1000, x_err = 0
    assert o.tobytes() == np.zeros(1, engine.TREND_DTYPE).tobytes()   # nothing seen before
    e = _entry(t, 1, 2)
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (1000.0, 0.0, 0.0, 0.0, 1, 1)
    o = t.window(edges_of((G(1), G(2), 1, 1, 3000)), NOOB)            # x_lat = 3000, x_err = 2^20
    assert o[0]["windows_seen"] == 1 and o[0]["base_mean_us"] == np.float32(1.0)
    assert o[0]["lat_dev"] == np.float32(2000 / 1000) and o[0]["err_dev"] == np.float32((1 << 20) / 10486)   # the floors
    e = _entry(t, 1, 2)
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (2000.0, 1000.0, 2.0 ** 19, 2.0 ** 19, 2, 2)
    o = t.window(edges_of((G(1), G(2), 4, 1, 8000)), NOOB)            # x_lat = 2000, x_err = 2^18
    assert o[0]["windows_seen"] == 2 and o[0]["base_mean_us"] == np.float32(2.0)
    assert o[0]["lat_dev"] == 0.0 and o[0]["err_dev"] == np.float32((2.0 ** 18 - 2.0 ** 19) / 2.0 ** 19) == np.float32(-0.5)
    e = _entry(t, 1, 2)
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (2000.0, 500.0, 393216.0, 393216.0, 3, 3)
    assert t.stats == dict(windows=3, entries=1, inserted=1, expired=0, dropped=0)


def test_a_group_edge_without_requests_neither_creates_nor_refreshes():
    t = GroupTrendRef(64, shift=1, warmup=1, ttl=2)
    t.window(edges_of((G(1), G(2), 0, 0, 0)), NOOB)                   # it folds alive-only rows only
    assert len(t.entries) == 0
    t.window(edges_of((G(1), G(2), 2, 0, 200)), NOOB)
    assert _entry(t, 1, 2)["last"] == 2
    o = t.window(edges_of((G(1), G(2), 0, 0, 0)), NOOB)               # the prior entry is reported, not refreshed
    assert o[0]["windows_seen"] == 1 and o[0]["lat_dev"] == 0 and o[0]["base_mean_us"] == np.float32(0.1)
    assert _entry(t, 1, 2)["last"] == 2 and _entry(t, 1, 2)["n"] == 1
    t.window(edges_of((G(1), G(2), 0, 0, 0)), NOOB)                   # w - last = 2 = ttl: expired
    assert len(t.entries) == 0 and t.stats["expired"] == 1


def test_x_err_of_u64_counts_does_not_overflow():
    e, c = (1 << 44) + 12345, (1 << 45) + 7
    assert float((np.uint64(e) << np.uint64(20)) // np.uint64(c)) != float((e << 20) // c)   # the naive u64 product wraps
    t = GroupTrendRef(64)
    t.window(edges_of((G(0), G(1), c, e, (1 << 64) - 1)), NOOB)
    ent = _entry(t, 0, 1)
    assert ent["err_mean"] == float((e << 20) // c) and ent["lat_mean"] == float(((1 << 64) - 1) // c)
    t2 = GroupTrendRef(64)
    t2.window(edges_of((G(0), G(1), 1, 0, (1 << 64) - 1)), NOOB)      # x_lat clamps at 2^52
    assert _entry(t2, 0, 1)["lat_mean"] == float(1 << 52)


def test_x_lat_is_taken_of_the_wrapped_sum():
    a, b, s = ref(REF_KNOWN, 0), ref(REF_KNOWN, 1), ref(REF_KNOWN, 2)
    rows = rows_of((a, s, 1, 0, (1 << 63) + 5), (b, s, 1, 0, (1 << 63) + 5))   # one workload: the u64 sum wraps to 10
    gmap = np.array([4, 4, NO], np.uint32)
    ge, _, _ = group_ref(rows, gmap, 8, 3, 4)
    assert len(ge) == 1 and int(ge["sum_ns"][0]) == 10 and int(ge["count"][0]) == 2
    t = GroupTrendRef(64)
    t.window(ge, NOOB)
    assert _entry(t, 4, (1 << 32) | 2)["lat_mean"] == 5.0


def test_an_outbound_ip_destination_keeps_its_entry_when_its_index_moves():
    ip = 0x0A000102
    t = GroupTrendRef(64, shift=1, warmup=1)
    t.window(edges_of((G(3), ref(REF_OBIP, 0), 1, 0, 1000)), np.array([ip, 0xC0A80001], np.uint32))
    key = (3 << 32) | ip
    assert _entry(t, 3, key)["lat_mean"] == 1000.0
    ob2 = np.array([0x01010101, 0x0A000001, ip], np.uint32)           # the same address at index 2, another one at index 0
    o = t.window(edges_of((G(3), ref(REF_OBIP, 0), 1, 0, 10), (G(3), ref(REF_OBIP, 2), 1, 0, 3000)), ob2)
    assert o[1]["windows_seen"] == 1 and o[1]["lat_dev"] == np.float32(2.0) and o[0]["windows_seen"] == 0
    assert _entry(t, 3, key)["n"] == 2 and _entry(t, 3, (3 << 32) | 0x01010101)["n"] == 1


def test_a_group_id_and_an_ungrouped_node_id_with_the_same_number_are_two_keys():
    dst = ref(REF_KNOWN, 9)
    t = GroupTrendRef(64)
    t.window(edges_of((G(5), dst, 1, 0, 100), (ref(REF_KNOWN, 5), dst, 1, 0, 700)), NOOB)
    assert [(int(e["from_key"]), int(e["to_key"])) for e in t.entries] == [(5, (1 << 32) | 9), ((1 << 32) | 5, (1 << 32) | 9)]
    assert [e["lat_mean"] for e in t.entries] == [100.0, 700.0]


def test_capacity_cut_and_vanished_workload_dependencies():
    t = GroupTrendRef(64, shift=1, warmup=1, ttl=4, max_entries=2)
    v = GroupVanishRef(t, silent_windows=1, min_seen=1, max_rows=1)
    w1 = edges_of((G(0), G(1), 1, 0, 10), (G(0), G(2), 1, 0, 10), (G(1), G(2), 1, 0, 10))
    _, lst, n = v.window(w1, NOOB)
    assert n == 0 and t.stats["dropped"] == 1 and [int(e["to_key"]) for e in t.entries] == [1, 2]   # the first two in key order
    _, lst, n = v.window(edges_of((G(0), G(1), 0, 0, 0), (G(1), G(2), 1, 0, 10)), NOOB)   # (0,1) alive-only, (0,2) gone, room for none
    assert n == 2 and len(lst) == 1                                   # max_rows cuts the list, not the count
    assert (int(lst[0]["from_key"]), int(lst[0]["to_key"]), int(lst[0]["row"])) == (0, 1, 0)   # the count == 0 group edge with its key
    v2 = GroupVanishRef(GroupTrendRef(64, warmup=1, ttl=4), silent_windows=1, min_seen=1)
    v2.window(w1, NOOB)
    _, lst, n = v2.window(edges_of((G(0), G(1), 0, 0, 0)), NOOB)
    assert n == 3 and lst["row"].tolist() == [0, NO_ROW, NO_ROW]
    _, lst, n = v2.window(edges_of((G(0), G(1), 0, 0, 0)), NOOB)      # listed once
    assert n == 0


def test_group_selection_reference():
    g = np.zeros(6, engine.GROUP_EDGE_DTYPE)
    g["score_max"] = np.array([0.5, 0.9, -0.0, 0.9, np.nan, 0.0], np.float32)
    g["count"] = [1, 0, 3, 2, 0, 0]
    tr = np.zeros(6, engine.TREND_DTYPE)
    tr["lat_dev"] = [1.0, 3.0, 2.0, 3.0, 0.0, np.nan]
    tr["windows_seen"] = [0, 0, 0, 4, 0, 0]
    assert list(ref_select_groups(g, None, "score", 0, 0.0)) == [0, 1, 2, 3, 5]           # NaN never, -0.0 >= 0.0
    assert list(ref_select_groups(g, None, "score", 3, float("-inf"))) == [1, 3, 0]       # ties by position
    assert list(ref_select_groups(g, None, "score", 5, float("-inf"))) == [1, 3, 0, 2, 5]
    assert list(ref_select_groups(g, tr, "lat_dev", 2, 0.0)) == [1, 3]
    assert list(ref_select_groups(g, tr, "lat_dev", 0, 2.0)) == [1, 2, 3]
    assert list(ref_select_groups(g, tr, "new", 0, 99.0)) == [0, 2]                       # requests, nothing seen; min_value ignored
    assert list(ref_select_groups(g, tr, "new", 1, 0.0)) == [0]


# ---- the ordering claim -------------------------------------------------------------------------------------------------------
def _obips(rng, n=40):
    return np.sort(rng.choice(np.arange(1, 1 << 32, 65537, dtype=np.uint64), n, replace=False)).astype(np.uint32)


def _map(kind, mk, n):
    """the three maps of tests/test_gpu_groups.py"""
    m = np.full(mk, NO, np.uint32)
    if kind == "blocks":
        m[:n] = np.arange(n) // 7
    elif kind == "one":
        m[:n] = 0
    return m


@pytest.mark.parametrize("seed", range(6))
def test_group_edges_are_strictly_ascending_in_their_workload_keys(seed):
    rng = np.random.default_rng(1500 + seed)
    mk, ml = int(rng.integers(8, 200)), int(rng.integers(1, 30))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 6 * mk)))
    obips = _obips(rng)
    mg = int(rng.integers(1, mk + 1))
    maps = [_random_map(rng, mk, mg), _random_map(rng, mk, mg, 1.0, block=7)] + [_map(k, mk, mk - 3) for k in ("none", "blocks", "one")]
    for gmap in maps:
        top = max(mg, int(gmap[gmap != NO].max()) + 1 if (gmap != NO).any() else 1)
        ge, _, _ = group_ref(rows, gmap, top, mk, ml)
        fk, tk = group_keys(ge, obips)
        assert strictly_ascending(fk, tk)
        GroupTrendRef(len(rows)).window(ge, obips)                     # (the reference asserts it too)
    ge, _, _ = group_ref(rows, _map("none", mk, mk), mk, mk, ml)       # nothing grouped: the edge keys, one type up
    efk, etk = TrendRef(1).window.__globals__["row_keys"](rows, obips)
    fk, tk = group_keys(ge, obips)
    assert (fk == efk + np.uint64(1 << 32)).all() and (tk == etk + np.uint64(1 << 32)).all()


# ---- the rollout ----------------------------------------------------------------------------------------------------------------
def test_a_rollout_resets_the_pod_baseline_and_not_the_workload_baseline():
    """workload 0 = pods 0..7, calling service node 20.  Pods 0..3 carry the traffic for warmup + 2 windows, then pods 4..7 (new
    pods, new ids): every pod-level row is a new dependency, the workload's group edge has the full history"""
    warmup, mk = 2, 24
    gmap = np.full(mk, NO, np.uint32); gmap[:8] = 0
    svc = ref(REF_KNOWN, 20)
    pod, grp = TrendRef(64, shift=1, warmup=warmup), GroupTrendRef(64, shift=1, warmup=warmup)
    pv, gv = [], []
    for w in range(warmup + 4):
        half = range(0, 4) if w < warmup + 2 else range(4, 8)
        lat = 1000 if w < warmup + 2 else 5000                        # a latency step at the switch
        rows = rows_of(*[(ref(REF_KNOWN, p), svc, 2, 0, 2 * lat) for p in half])
        ge, _, _ = group_ref(rows, gmap, 8, mk, 4)
        assert len(ge) == 1 and ge["from_ref"][0] == G(0) and ge["count"][0] == 8
        pv.append(pod.window(rows, NOOB)); gv.append(grp.window(ge, NOOB))
    sw = warmup + 2
    assert (pv[sw]["windows_seen"] == 0).all() and (pv[sw]["lat_dev"] == 0).all()      # "a new dependency", four times
    assert gv[sw]["windows_seen"][0] == sw and gv[sw]["lat_dev"][0] == np.float32(4000 / 1000)   # the history, and the step
    assert gv[sw]["base_mean_us"][0] == np.float32(1.0)
    assert pv[sw + 1]["windows_seen"].tolist() == [1] * 4 and gv[sw + 1]["windows_seen"][0] == sw + 1
    assert len(pod.entries) == 8 and len(grp.entries) == 1


# ---- the plans ------------------------------------------------------------------------------------------------------------------
group_trend_plan = plan_fixture("group_trend")


def _p(me, slots=1, ss=40, shift=0, warmup=0, ttl=0, maxe=0, lf=0, ef=0, res=0, vss=16, silent=0, seen=0, rows=0, cb=512):
    return (me, slots, ss, shift, warmup, ttl, maxe, lf, ef, res, vss, silent, seen, rows, cb)


EDGES = [1, 2, 255, 2048, 4097, 1 << 15, 1_250_000, (1 << 24) + 3, 1 << 31]


def test_plan_sizes_fit_every_window(group_trend_plan):
    lines = [_p(me, slots) for me in EDGES for slots in (1, 3, 8)] + [_p(me, 1, maxe=m) for me in EDGES for m in (1, 2, 7, 33, 1 << 20)]
    for r in group_trend_plan(lines):
        assert r["rc"] == 0 and r["trend_size"] == 16 and r["group_edge_size"] == 80
        me, cap = r["max_edges"], r["entries"]
        assert cap == r["max_entries"] >= 1 and cap <= 1 << 31
        assert 1 <= r["wgs"] <= r["max_wgs"] == 1024
        assert r["soa_bytes"] >= 56 * cap and r["soa_bytes"] % 256 == 0
        assert r["rows_bytes"] >= 16 * me and r["rows_bytes"] % 256 == 0     # a trend row for every group edge a slot's window can have
        assert r["total_bytes"] == 2 * r["soa_bytes"] + r["ctl_bytes"] + r["blk_bytes"] + r["thread_bytes"] + r["slots"] * r["rows_bytes"]
        check_layout(r, {"soa0": 56 * cap, "soa1": 56 * cap, "ctl": 64, "blk": 16 * r["wgs"], "thread": 16 * 256 * r["wgs"], "rows": 16 * me},
                     per_slot=("rows",))
        check_soa(r)
        if r["wgs"] < 1024:                                           # B + E merged elements, about eight per thread
            assert r["wgs"] * 256 * r["per_thread"] >= cap + me
        v = r["van"]                                                  # the default list: k8_count_v's counts over the same grid
        assert v["rc"] == 0 and v["max_rows"] == v["rows"] == min(65536, cap) and v["min_seen"] == r["warmup"] and v["silent_windows"] == 1
        check_layout(v, {"thread": 4 * 256 * r["wgs"], "blk": 4 * r["wgs"], "list": 64 * v["max_rows"], "count": 8}, per_slot=("list", "count"))
        s = r["sel"]                                                  # K7's scratch over max_edges keys, indices, MAX_K rows of staging
        assert s["stage_rows"] == s["select_max_k"] == engine.SELECT_MAX_K and s["key_bytes"] == 4 * me
        assert 1 <= s["wgs"] <= 1024 and (s["wgs"] == 1024 or s["wgs"] * 2048 >= me)
        check_layout(s, {"stage": 80 * engine.SELECT_MAX_K, "ctr": 512, "idx": 4 * me, "sel": s["scratch_bytes"]})
        k7 = {"pairs": 8 * engine.SELECT_MAX_K, "state": 8 + 4 * 8, "blk": 16 * s["wgs"], "hist": 1024 * s["wgs"], "keys": 4 * me}
        check_layout(s, k7, align=8, layout="k7_layout", total="scratch_bytes", tail_align=4)
    c3, = group_trend_plan([_p(1_250_000)])
    assert c3["entries"] == 2_500_000 and c3["wgs"] == 1024 and c3["total_bytes"] < 320 << 20
    small, = group_trend_plan([_p(1 << 15)])
    assert small["entries"] == 1 << 16 and small["wgs"] == 48        # the GPU tests' engines: the merge spans 48 workgroups


def test_plan_defaults_and_invalid_parameters(group_trend_plan):
    d, = group_trend_plan([_p(1000)])
    assert (d["shift"], d["warmup"], d["ttl"], d["max_entries"], d["lat_floor_ns"], d["err_floor"]) == (4, 4, 64, 2000, 1000, 10486)
    z, = group_trend_plan([_p(0)])
    assert z["max_entries"] == 2 and z["rows_bytes"] >= 16
    big, = group_trend_plan([_p(1 << 31)])
    assert big["max_entries"] == 1 << 31
    k, = group_trend_plan([_p(1000, shift=10, warmup=1, ttl=1, maxe=5, lf=7, ef=9)])
    assert (k["shift"], k["warmup"], k["ttl"], k["max_entries"], k["lat_floor_ns"], k["err_floor"]) == (10, 1, 1, 5, 7, 9)
    bad = group_trend_plan([_p(1000, shift=11), _p(1000, ss=36), _p(1000, ss=48), _p(1000, res=1), _p(1000, maxe=(1 << 31) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
    # the vanished list against the group trend's resolved parameters: silent < ttl, max_rows <= max_entries, the struct size
    v = group_trend_plan([_p(1000, ttl=3, silent=3), _p(1000, ttl=3, silent=2), _p(1000, maxe=5, rows=6), _p(1000, maxe=5, rows=5),
                          _p(1000, vss=12), _p(1000, warmup=3, seen=0)])
    assert [r["van"]["rc"] for r in v] == [engine.SG_EINVAL, 0, engine.SG_EINVAL, 0, engine.SG_EINVAL, 0]
    assert v[5]["van"]["min_seen"] == 3 and v[3]["van"]["max_rows"] == 5
    assert C.sizeof(engine.SgTrendParams) == 40 and C.sizeof(engine.SgVanishedParams) == 16


# ---- the front end, against the recording stand-in ------------------------------------------------------------------------------
U4, same, pattern, INF = front.U4, front.same, front.pattern, front.INF
H, I, F, O, S, SO, Out = front.H, front.I, front.F, front.O, front.S, front.SO, front.Out
NEW_ABI = {
    "sg_set_group_trend": [H, S], "sg_set_group_vanished": [H, S],
    "sg_window_group_trend": front._INDEXED(engine.TREND_DTYPE),
    "sg_group_trend_entries": front._COUNTED(engine.TREND_ENTRY_DTYPE), "sg_window_group_vanished": front._COUNTED(engine.VANISHED_DTYPE),
    "sg_window_group_trend_buffer": [H, O], "sg_window_group_vanished_buffer": [H, O, O], "sg_group_trend_stats_get": [H, SO],
    "sg_window_groups_top": [H, I, I, F, Out(engine.GROUP_EDGE_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_groups_select": [H, I, I, F, I, I, I, I, I],
}
_TREND = [("shift", 4), ("warmup", 4), ("ttl", 64), ("max_entries", 0), ("lat_floor_ns", 1000), ("err_floor", 10486)]


g = front.abi_fixture(NEW_ABI)


def _trend_bytes(**over):
    v = [over.get("struct_size", 40)] + [over.get(f, d) for f, d in _TREND] + [over.get("reserved", 0)]
    return struct.pack("<4I2Q2I", *v)


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 10
    for name, kinds in NEW_ABI.items():
        assert len(engine._SIGNATURES[name][1]) == len(kinds), name


def test_set_group_trend_and_set_group_vanished(g):
    assert g.set_group_trend() is None and g.set_group_trend(dict(shift=2), ttl=9) is None and g.set_group_trend(None) is None
    assert g._l.take() == [("sg_set_group_trend", "h", _trend_bytes()), ("sg_set_group_trend", "h", _trend_bytes(shift=2, ttl=9)),
                           ("sg_set_group_trend", "h", None)]
    assert g.set_group_vanished() is None and g.set_group_vanished(silent_windows=2, max_rows=7) is None and g.set_group_vanished(None) is None
    assert g._l.take() == [("sg_set_group_vanished", "h", struct.pack("<4I", 16, 0, 0, 0)),
                           ("sg_set_group_vanished", "h", struct.pack("<4I", 16, 2, 0, 7)), ("sg_set_group_vanished", "h", None)]
    with pytest.raises(TypeError) as ei:
        g.set_group_trend(None, shift=1)
    assert str(ei.value) == "set_group_trend(None) switches the group trend off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_trend(zzz=1)
    assert str(ei.value) == "unknown group trend parameters: ['zzz']"
    with pytest.raises(TypeError) as ei:
        g.set_group_vanished(None, max_rows=1)
    assert str(ei.value) == "set_group_vanished(None) switches the list off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_vanished(reserved=0)
    assert str(ei.value) == "unknown group vanished parameters: ['reserved']"
    assert g._l.take() == []
    g._l.script = {"sg_set_group_trend": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"sg_set_group_trend: the groups are off (sg_set_groups)")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_trend()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: sg_set_group_trend: the groups are off (sg_set_groups)"


def test_window_group_trend_is_an_indexed_readback(g):
    cfn, dt = "sg_window_group_trend", engine.TREND_DTYPE
    same(g.window_group_trend(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_trend(index=None), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(g.window_group_trend(index=[]), dt, pattern(dt, 0))
    assert g._l.take() == []
    g._l.script[cfn] = dict(out=[2])
    same(g.window_group_trend([2, 0]), dt, pattern(dt, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]


def test_group_trend_entries_stats_and_buffers(g):
    g._l.script = {"sg_group_trend_entries": dict(out=[3]), "sg_group_trend_stats_get": dict(fields=dict(windows=4, dropped=2)),
                   "sg_window_group_trend_buffer": dict(out=[0x1000]), "sg_window_group_vanished_buffer": dict(out=[0x2000, 0x3000])}
    same(g.group_trend_entries(), engine.TREND_ENTRY_DTYPE, pattern(engine.TREND_ENTRY_DTYPE, 3))
    s = g.group_trend_stats()
    assert type(s) is engine.SgTrendStats and (s.windows, s.entries, s.dropped) == (4, 0, 2)
    assert g.window_group_trend_buffer() == 0x1000 and g.window_group_vanished_buffer() == (0x2000, 0x3000)
    assert g._l.take() == [("sg_group_trend_entries", "h", None, 0, "out"), ("sg_group_trend_entries", "h", "buf", 3, "out"),
                           ("sg_group_trend_stats_get", "h", "out:SgTrendStats"), ("sg_window_group_trend_buffer", "h", "out"),
                           ("sg_window_group_vanished_buffer", "h", "out", "out")]
    g._l.script = {"sg_window_group_trend_buffer": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_trend_buffer()
    assert str(ei.value) == "servicegraph rc=-71: off"


@pytest.mark.parametrize("max_edges,rows", [(100, 200), (40000, 65536), (0, 2)])
def test_window_group_vanished_clips_to_what_the_switches_recorded(g, max_edges, rows):
    g.max_edges = max_edges
    g.set_group_trend(max_entries=0)
    g.set_group_vanished()
    g._l.take()
    g._l.script["sg_window_group_vanished"] = dict(out=[rows + 3])
    got, n = g.window_group_vanished(with_count=True)
    assert g._l.take() == [("sg_window_group_vanished", "h", None, 0, "out"), ("sg_window_group_vanished", "h", "buf", rows + 3, "out")]
    same(got, engine.VANISHED_DTYPE, pattern(engine.VANISHED_DTYPE, rows))
    assert n == rows + 3
    g.set_group_vanished(max_rows=3)
    assert len(g.window_group_vanished()) == 3


def test_the_edge_and_the_group_switches_keep_their_own_records(g):
    g.set_trend(max_entries=4); g.set_vanished()
    g.set_group_trend(max_entries=9); g.set_group_vanished()
    g._l.script = {"sg_window_vanished": dict(out=[20]), "sg_window_group_vanished": dict(out=[20])}
    assert len(g.window_vanished()) == 4 and len(g.window_group_vanished()) == 9


def test_window_groups_top_and_select(g):
    cfn = "sg_window_groups_top"
    g._l.script = {cfn: dict(out=[5, 6])}
    rows, idx, n = g.window_groups_top(3, 0.5, by="err_dev")          # cap = k: 5 selected, 3 fit
    assert g._l.take() == [(cfn, "h", 2, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, engine.GROUP_EDGE_DTYPE, pattern(engine.GROUP_EDGE_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 6 and type(n) is int
    rows, idx, n = g.window_groups_top(0)                             # k = 0, cap=None: max_edges; score; -inf
    assert g._l.take() == [(cfn, "h", 0, 0, INF, "buf", "buf", 100, "out", "out")]
    assert len(rows) == len(idx) == 5
    rows, idx, n = g.window_groups_top(8, cap=1, by="new")
    assert g._l.take() == [(cfn, "h", 3, 8, INF, "buf", "buf", 1, "out", "out")]
    assert len(rows) == len(idx) == 1
    for bad in ("x", 2, "in_lat_dev"):                                # SG_SEL_*'s names, never a number or a node key
        with pytest.raises(ValueError) as ei:
            g.window_groups_top(3, by=bad)
        assert str(ei.value) == f"by must be one of ['err_dev', 'lat_dev', 'new', 'score'], not {bad!r}"
    assert g._l.take() == []
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"group selection by a trend key: the group trend is off (sg_set_group_trend)")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_groups_top(3, by="lat_dev")
    assert str(ei.value) == "servicegraph rc=-71: group selection by a trend key: the group trend is off (sg_set_group_trend)"
    g._l.take()
    assert g.window_groups_select(3, 0.5, 0x1000, 0x2000, 8, 0x3000, stream=0x4000) is None
    assert g.window_groups_select(0, 1.5, 0, 0x2000, 8, 0x3000, by="lat_dev") is None
    assert g._l.take() == [("sg_window_groups_select", "h", 0, 3, 0.5, 0x1000, 0x2000, 8, 0x3000, 0x4000),
                           ("sg_window_groups_select", "h", 1, 0, 1.5, None, 0x2000, 8, 0x3000, None)]


def test_the_stage_adds_no_struct_and_no_constant_set():
    twins = {n: v for n, v in vars(engine).items() if (n.startswith("Sg") and isinstance(v, type) and issubclass(v, C.Structure))
             or (n.endswith("_DTYPE") and isinstance(v, np.dtype))}
    assert all(any(v is t for t in LAYOUTS.values()) for v in twins.values()) and len(twins) == len(LAYOUTS) == 23
    assert engine.SEL_BY == dict(score=0, lat_dev=1, err_dev=2, new=3) and engine.ABI_VERSION == 6
    st = engine._STAGES
    assert st["group_trend"].struct is st["trend"].struct is engine.SgTrendParams and st["group_trend"].defaults is engine.TREND_DEFAULTS
    assert st["group_vanished"].struct is st["vanished"].struct is engine.SgVanishedParams and st["group_vanished"].defaults is engine.VANISHED_DEFAULTS


# ---- GraphDS: the switches forwarded, group ids resolved back to owner UIDs (the recording stand-in engine of host_capi.cpp) ----
def test_graphds_workload_baselines_against_the_stand_in_engine():
    from alaz_amd import hostlib
    ds = hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")                  # node 1, workload 1 = sts-q
    assert ds.set_workload_trend(shift=3, warmup=2, ttl=9) == 0 and ds.set_workload_trend() == 0
    assert ds.set_workload_vanished(silent_windows=2, max_rows=2) == 0
    t = ds.workload_trends()
    assert t.dtype == engine.TREND_DTYPE and t["windows_seen"].tolist() == [1, 2, 3, 4] and t["lat_dev"].tolist() == [0.5] * 4
    rows, idx = ds.workload_top(engine.SEL_BY["lat_dev"], 5, 1.5)
    assert idx.tolist() == [3, 0] and rows["count"].tolist() == [9, 4] and rows["score_max"].tolist() == [0.75, 0.5]
    assert [(r["from_type"], r["from_uid"], r["to_type"], r["to_uid"]) for r in rows] == \
        [(b"workload", b"sts-q", b"workload", b"dep-a"), (b"workload", b"dep-a", b"pod", b"pod-0")]
    rows, idx = ds.workload_top(engine.SEL_BY["score"], 0)            # k = 0: the count first, then the rows
    assert idx.tolist() == [3, 0] and len(rows) == 2
    v = ds.workload_vanished()                                        # three counted, max_rows = 2 held
    assert len(v) == 2 and v["from_key"].tolist() == [1, (1 << 32) | 7] and v["to_key"].tolist() == [0, (3 << 32) | 0x0A000001]
    assert v["from_uid"].tolist() == [b"sts-q", b""] and v["to_uid"].tolist() == [b"dep-a", b""]     # other key types keep their key
    assert v["row"].tolist() == [2, 0xFFFFFFFF] and v["n"].tolist() == [5, 6] and v["lat_mean"].tolist() == [1000.0, 2000.0]
    bits = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])   # noqa: E731
    assert [tuple(int(x) for x in r) for r in ds.mock_k15_ops()] == \
        [(1, 3, 2, 9), (1, 0, 0, 0), (2, 2, 0, 2)] + [(3, 1, 5, bits(1.5))] * 2 + [(3, 0, 0, bits(float("-inf")))] * 4
    # (the twin asks for the count, then for the rows: two WorkloadTop calls each; with k = 0 WorkloadTop itself asks the engine twice)
