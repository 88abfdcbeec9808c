"""CPU tests of the per-node baselines (K10): the numpy reference tests/node_trend_ref.py against hand-computed sequences, the node
selection's reference, and the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage node_trend) — parameter checks and
defaults, and memory for every window an engine can close."""
import ctypes as C
import os

import numpy as np

from alaz_amd import engine
from tests.helpers import ref
from tests.host_scaffold import node_trend_rows_of as rows_of
from tests.node_trend_ref import NodeTrendRef, node_samples, ref_select_nodes, x_err
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests.trend_ref import REF_KNOWN, REF_LABEL, REF_OBIP

HERE = os.path.dirname(os.path.abspath(__file__))

A, B_, C_ = ref(REF_KNOWN, 1), ref(REF_KNOWN, 2), ref(REF_KNOWN, 3)
NOOB = np.zeros(0, np.uint32)


def _win(t, rows, obips=NOOB):
    n = nodes_ref(rows)
    return n, t.window(n, obips)


def _entry(t, nk, side):
    e = t.entries[(t.entries["from_key"] == nk) & (t.entries["to_key"] == side)]
    return e[0] if len(e) else None


def test_dtype_matches_the_header():
    assert engine.NODE_TREND_DTYPE.itemsize == 32
    assert [engine.NODE_TREND_DTYPE.fields[f][1] for f in ("in_lat_dev", "out_err_dev", "in_base_mean_us", "in_seen", "out_seen")] == [0, 12, 16, 24, 28]
    assert engine.NSEL_BY == dict(score=0, in_lat_dev=1, in_err_dev=2, out_lat_dev=3, out_err_dev=4, new=5)


def test_samples_are_the_two_sides_in_key_order():
    n = nodes_ref(rows_of((A, B_, 2, 1, 2000), (B_, C_, 3, 0, 900)))
    s = node_samples(n)
    assert list(s["ref"]) == [A, A, B_, B_, C_, C_] and list(s["side"]) == [0, 1] * 3
    assert list(s["count"]) == [0, 2, 2, 3, 3, 0] and list(s["err"]) == [0, 1, 1, 0, 0, 0]


def test_pure_caller_and_pure_callee_have_one_side_each():
    t = NodeTrendRef(64, shift=1, warmup=1)
    n, o = _win(t, rows_of((A, B_, 2, 0, 2000)))                     # A only calls, B only receives; x = 1000
    assert list(n["ref"]) == [A, B_]
    assert len(t.entries) == 2
    assert _entry(t, A, 0) is None and _entry(t, B_, 1) is None
    ea, eb = _entry(t, A, 1), _entry(t, B_, 0)
    assert (ea["lat_mean"], ea["n"], eb["lat_mean"], eb["n"]) == (1000.0, 1, 1000.0, 1)
    assert o.tobytes() == np.zeros(2, engine.NODE_TREND_DTYPE).tobytes()   # nothing seen before
    n, o = _win(t, rows_of((A, B_, 1, 1, 3000)))                     # x = 3000, one error of one
    a, b = o[0], o[1]
    assert a["out_seen"] == 1 and a["in_seen"] == 0 and a["out_lat_dev"] == np.float32(2.0) and a["in_lat_dev"] == 0
    assert a["out_base_mean_us"] == np.float32(1.0) and a["in_base_mean_us"] == 0
    assert b["in_seen"] == 1 and b["out_seen"] == 0 and b["in_lat_dev"] == np.float32(2.0)
    assert b["in_err_dev"] == np.float32((1 << 20) / 10486)
    e = _entry(t, A, 1)
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (2000.0, 1000.0, 2.0 ** 19, 2.0 ** 19, 2, 2)


def test_self_loop_counts_on_both_sides():
    t = NodeTrendRef(64, shift=2, warmup=1)
    _win(t, rows_of((A, A, 4, 1, 4000), (A, B_, 1, 0, 9000)))
    ei, eo = _entry(t, A, 0), _entry(t, A, 1)
    assert ei["lat_mean"] == 1000.0 and ei["err_mean"] == float((1 << 20) // 4)
    assert eo["lat_mean"] == float(13000 // 5) and eo["err_mean"] == float((1 << 20) // 5)
    n, o = _win(t, rows_of((A, A, 4, 0, 8000)))
    assert o[0]["in_lat_dev"] == np.float32((2000 - 1000) / 1000) and o[0]["out_lat_dev"] == np.float32((2000 - 2600) / 1000)
    assert o[0]["in_seen"] == o[0]["out_seen"] == 1


def test_alive_only_node_neither_creates_nor_refreshes():
    t = NodeTrendRef(64, shift=1, warmup=1, ttl=2)
    _win(t, rows_of((A, B_, 0, 0, 0)))                               # alive-only: both nodes, no sample
    assert len(t.entries) == 0
    _win(t, rows_of((A, B_, 2, 0, 200)))
    assert len(t.entries) == 2
    n, o = _win(t, rows_of((A, B_, 0, 0, 0)))                        # prior entries reported, not refreshed
    assert o[0]["out_seen"] == 1 and o[0]["out_lat_dev"] == 0 and o[0]["out_base_mean_us"] == np.float32(0.1)
    assert _entry(t, A, 1)["last"] == 2
    _win(t, rows_of((A, B_, 0, 0, 0)))                               # w - last = 2 = ttl: expired
    assert len(t.entries) == 0 and t.stats["expired"] == 2


def test_outbound_ip_node_keeps_its_baseline_when_its_index_moves():
    ip = 0x0A000102
    t = NodeTrendRef(64, shift=1, warmup=1)
    ob1 = np.array([ip, 0xC0A80001], np.uint32)
    _win(t, rows_of((A, ref(REF_OBIP, 0), 1, 0, 1000)), ob1)
    nk = (REF_OBIP << 32) | ip
    assert _entry(t, nk, 0)["lat_mean"] == 1000.0
    ob2 = np.array([0x01010101, 0x0A000001, ip], np.uint32)          # the same IP at index 2
    n, o = _win(t, rows_of((A, ref(REF_OBIP, 2), 1, 0, 3000), (ref(REF_OBIP, 0), A, 1, 0, 10)), ob2)
    assert list(n["ref"]) == [A, ref(REF_OBIP, 0), ref(REF_OBIP, 2)]
    assert o[2]["in_seen"] == 1 and o[2]["in_lat_dev"] == np.float32(2.0)
    assert o[1]["out_seen"] == 0 and o[1]["in_seen"] == 0             # another IP: new
    assert _entry(t, nk, 0)["n"] == 2 and _entry(t, (REF_OBIP << 32) | 0x01010101, 1)["n"] == 1


def test_labels_sort_after_known_nodes():
    t = NodeTrendRef(64)
    _win(t, rows_of((A, ref(REF_LABEL, 5), 1, 0, 10)))
    assert list(t.entries["from_key"]) == [A, (REF_LABEL << 32) | 5] and list(t.entries["to_key"]) == [1, 0]


def test_warmup_holds_the_deviations_back():
    t = NodeTrendRef(64, shift=1, warmup=3)
    for i, x in enumerate([1000, 1000, 1000, 5000]):
        n, o = _win(t, rows_of((A, B_, 1, 0, x)))
        if i < 3:
            assert o[0]["out_lat_dev"] == 0 and o[1]["in_lat_dev"] == 0 and o[0]["out_seen"] == i
    assert o[0]["out_seen"] == 3 and o[0]["out_lat_dev"] == np.float32(4.0)


def test_ttl_expiry_and_reentry():
    t = NodeTrendRef(64, ttl=2)
    _win(t, rows_of((A, B_, 1, 0, 10)))
    _win(t, rows_of((B_, C_, 1, 0, 10)))                             # A's out side: w - last = 1, kept
    assert _entry(t, A, 1) is not None
    _win(t, rows_of((B_, C_, 1, 0, 10)))                             # = 2: expired
    assert _entry(t, A, 1) is None and _entry(t, B_, 0) is None and t.stats["expired"] == 2
    n, o = _win(t, rows_of((A, B_, 1, 0, 10)))
    assert o[0]["out_seen"] == 0 and _entry(t, A, 1)["n"] == 1       # back as new


def test_capacity_cut_in_key_order():
    t = NodeTrendRef(64, max_entries=3)
    _win(t, rows_of((A, B_, 1, 0, 10), (B_, C_, 1, 0, 10)))         # samples: A1, B0, B1, C0 -> the first three go in
    assert [(int(e["from_key"]), int(e["to_key"])) for e in t.entries] == [(A, 1), (B_, 0), (B_, 1)]
    assert t.stats["inserted"] == 3 and t.stats["dropped"] == 1
    _win(t, rows_of((A, B_, 1, 0, 10), (B_, C_, 1, 0, 10)))
    assert t.stats["dropped"] == 2 and len(t.entries) == 3


def test_x_err_is_exact_for_large_counts():
    e, c = (1 << 44) + 12345, (1 << 45) + 7
    assert x_err([e], [c])[0] == float(((e << 20) // c))
    assert x_err([e], [c])[0] != float((np.uint64(e) << np.uint64(20)) // np.uint64(c))   # the u64 product would wrap
    n = np.zeros(1, engine.NODE_DTYPE)
    n["ref"] = A; n["in_count"] = c; n["in_err"] = e; n["in_sum_ns"] = (1 << 64) - 1
    t = NodeTrendRef(64)
    t.window(n, NOOB)
    ent = _entry(t, A, 0)
    assert ent["err_mean"] == float((e << 20) // c) and ent["lat_mean"] == float(((1 << 64) - 1) // c)
    n["in_count"] = 1
    t.window(n, NOOB)
    assert _entry(t, A, 0)["n"] == 2                                 # x_lat clamps at 2^52
    t2 = NodeTrendRef(64); t2.window(n, NOOB)
    assert _entry(t2, A, 0)["lat_mean"] == float(1 << 52)


def test_node_selection_reference():
    n = np.zeros(6, engine.NODE_DTYPE)
    n["ref"] = np.arange(6)
    n["score"] = np.array([0.5, 0.9, -0.0, 0.9, np.nan, 0.0], np.float32)
    n["out_count"] = [1, 0, 0, 2, 0, 0]; n["in_count"] = [0, 0, 3, 0, 0, 0]
    tr = np.zeros(6, engine.NODE_TREND_DTYPE)
    tr["in_lat_dev"] = [1.0, 3.0, 2.0, 3.0, 0.0, np.nan]
    tr["out_seen"] = [0, 0, 0, 4, 0, 0]
    assert list(ref_select_nodes(n, None, "score", 0, 0.0)) == [0, 1, 2, 3, 5]   # NaN never, -0.0 >= 0.0
    assert list(ref_select_nodes(n, None, "score", 3, float("-inf"))) == [1, 3, 0]
    assert list(ref_select_nodes(n, None, "score", 5, float("-inf"))) == [1, 3, 0, 2, 5]   # -0.0 == +0.0: by position
    assert list(ref_select_nodes(n, tr, "in_lat_dev", 2, 0.0)) == [1, 3]
    assert list(ref_select_nodes(n, tr, "in_lat_dev", 0, 2.0)) == [1, 2, 3]
    assert list(ref_select_nodes(n, tr, "new", 0, 99.0)) == [0, 2]   # requests, nothing seen; min_value ignored
    assert list(ref_select_nodes(n, tr, "new", 1, 0.0)) == [0]


node_trend_plan = plan_fixture("node_trend")


def _p(nc, slots=1, ss=40, shift=0, warmup=0, ttl=0, maxe=0, lf=0, ef=0, res=0):
    return (nc, slots, ss, shift, warmup, ttl, maxe, lf, ef, res)


NCAPS = [1, 2, 255, 1024, 1076, 15_000, 1 << 17, (1 << 20) + 3, 1 << 24, 0x3FFFFFFF + 256 + 4096]


def test_plan_sizes_fit_every_window(node_trend_plan):
    lines = [_p(nc, slots) for nc in NCAPS for slots in (1, 3, 8)] + [_p(nc, 1, maxe=m) for nc in NCAPS for m in (1, 2, 7, 33, 1 << 20)]
    for r in node_trend_plan(lines):
        assert r["rc"] == 0 and r["node_trend_size"] == 32
        nc, C_ = r["ncap"], r["entries"]
        assert C_ == r["max_entries"] >= 1 and C_ <= 1 << 31
        assert 1 <= r["wgs"] <= r["max_wgs"] == 1024
        assert r["soa_bytes"] >= 56 * C_ and r["soa_bytes"] % 256 == 0
        assert r["rows_bytes"] >= 32 * nc and r["rows_bytes"] % 256 == 0     # every node row of every window a slot can close
        assert r["blk_bytes"] >= 16 * r["wgs"] and r["thread_bytes"] >= 16 * 256 * r["wgs"] and r["ctl_bytes"] >= 64
        assert r["total_bytes"] == 2 * r["soa_bytes"] + r["ctl_bytes"] + r["blk_bytes"] + r["thread_bytes"] + r["slots"] * r["rows_bytes"]
        check_layout(r, {"soa0": 56 * C_, "soa1": 56 * C_, "ctl": 64, "blk": 16 * r["wgs"], "thread": 16 * 256 * r["wgs"], "rows": 32 * nc}, per_slot=("rows",))
        check_soa(r)
        if r["wgs"] < 1024:                                           # B + 2N merged elements, about eight per thread
            assert r["wgs"] * 256 * r["per_thread"] >= C_ + 2 * nc
    big = {(r["ncap"], r["slots"]): r for r in node_trend_plan([_p(NCAPS[-1], 3)])}[(NCAPS[-1], 3)]
    assert big["entries"] == 1 << 31 and big["wgs"] == 1024          # the largest window: the cap, every workgroup
    c3, = node_trend_plan([_p(15_000)])
    assert c3["entries"] == 60_000 and c3["wgs"] == 44 and c3["total_bytes"] < 8 << 20
    four, = node_trend_plan([_p(1076)])
    assert four["entries"] == 4304 and four["wgs"] == 4


def test_plan_defaults_and_invalid_parameters(node_trend_plan):
    d, = node_trend_plan([_p(1000)])
    assert (d["shift"], d["warmup"], d["ttl"], d["max_entries"], d["lat_floor_ns"], d["err_floor"]) == (4, 4, 64, 4000, 1000, 10486)
    z, = node_trend_plan([_p(0)])
    assert z["max_entries"] == 4
    k, = node_trend_plan([_p(1000, shift=10, warmup=1, ttl=1, maxe=5, lf=7, ef=9)])
    assert (k["shift"], k["warmup"], k["ttl"], k["max_entries"], k["lat_floor_ns"], k["err_floor"]) == (10, 1, 1, 5, 7, 9)
    bad = node_trend_plan([_p(1000, shift=11), _p(1000, ss=36), _p(1000, ss=48), _p(1000, res=1), _p(1000, maxe=(1 << 31) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
    ok, = node_trend_plan([_p(1000, maxe=1 << 31)])
    assert ok["rc"] == 0
    assert C.sizeof(engine.SgTrendParams) == 40
