"""CPU tests of the per-edge baselines (K8): the numpy reference tests/trend_ref.py against hand-computed sequences, and the plan
in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage trend) — parameter checks and defaults, and memory for every window an
engine can close."""
import ctypes as C
import os

import numpy as np

from alaz_amd import engine
from tests.helpers import ref
from tests.host_scaffold import trend_rows_of as rows_of
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests.trend_ref import REF_KNOWN, REF_LABEL, REF_OBIP, TrendRef, ref_keys, row_keys, strictly_ascending

HERE = os.path.dirname(os.path.abspath(__file__))

A, B_, C_ = ref(REF_KNOWN, 1), ref(REF_KNOWN, 2), ref(REF_KNOWN, 3)
NOOB = np.zeros(0, np.uint32)


def test_dtypes_match_the_header():
    assert engine.TREND_DTYPE.itemsize == 16 and engine.TREND_ENTRY_DTYPE.itemsize == 56
    assert C.sizeof(engine.SgTrendParams) == 40 and C.sizeof(engine.SgTrendStats) == 40
    assert engine.SgTrendParams.max_entries.offset == 16 and engine.SgTrendParams.err_floor.offset == 32
    assert engine.TREND_ENTRY_DTYPE.fields["n"][1] == 48 and engine.TREND_DTYPE.fields["windows_seen"][1] == 12


def test_ewma_steps_with_shift_1():
    t = TrendRef(64, shift=1, warmup=1)
    o = t.window(rows_of((A, B_, 2, 0, 2000)), NOOB)                 # x = 1000
    assert o["windows_seen"][0] == 0 and o["lat_dev"][0] == 0 and o["base_mean_us"][0] == 0
    e = t.entries[0]
    assert (e["lat_mean"], e["lat_dev"], e["n"], e["last"]) == (1000.0, 0.0, 1, 1)
    o = t.window(rows_of((A, B_, 1, 1, 3000)), NOOB)                 # x = 3000, one error of one
    assert o["windows_seen"][0] == 1 and o["base_mean_us"][0] == np.float32(1.0)
    assert o["lat_dev"][0] == np.float32(2.0)                        # (3000 - 1000) / max(0, 1000)
    assert o["err_dev"][0] == np.float32((1 << 20) / 10486)          # (2^20 - 0) / max(0, 10486)
    e = t.entries[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (2000.0, 1000.0, 2.0 ** 19, 2.0 ** 19, 2, 2)
    o = t.window(rows_of((A, B_, 4, 0, 8000)), NOOB)                 # x = 2000
    assert o["lat_dev"][0] == 0 and o["windows_seen"][0] == 2 and o["err_dev"][0] == np.float32(-1.0)
    e = t.entries[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"]) == (2000.0, 500.0, 2.0 ** 18, 2.0 ** 19)


def test_ewma_steps_with_shift_4():
    t = TrendRef(64, shift=4, warmup=1, lat_floor_ns=50)
    t.window(rows_of((A, B_, 1, 0, 1000)), NOOB)
    o = t.window(rows_of((A, B_, 1, 0, 2600)), NOOB)
    assert o["lat_dev"][0] == np.float32(1600 / 50)
    e = t.entries[0]
    assert (e["lat_mean"], e["lat_dev"]) == (1100.0, 100.0)          # 1000 + 1600 / 16, 0 + 1600 / 16
    o = t.window(rows_of((A, B_, 1, 0, 1100)), NOOB)
    assert o["lat_dev"][0] == 0
    e = t.entries[0]
    assert (e["lat_mean"], e["lat_dev"]) == (1100.0, 93.75)          # 100 + (0 - 100) / 16
    # x_lat saturates at 2^52, x_err is in units of 2^-20 (integer divisions)
    t2 = TrendRef(64, shift=4)
    t2.window(rows_of((A, B_, 1, 0, (1 << 63) + 5), (A, C_, 3, 1, 10)), NOOB)
    assert t2.entries["lat_mean"][0] == 2.0 ** 52 and t2.entries["lat_mean"][1] == 3.0 and t2.entries["err_mean"][1] == float((1 << 20) // 3)


def test_warmup_holds_the_deviations_back():
    t = TrendRef(64, shift=2, warmup=3)
    seen = []
    for x in (1000, 5000, 9000, 20000):
        o = t.window(rows_of((A, B_, 1, 0, x)), NOOB)
        seen.append((int(o["windows_seen"][0]), float(o["lat_dev"][0])))
    assert [s for s, _ in seen] == [0, 1, 2, 3]
    assert [d for _, d in seen[:3]] == [0.0, 0.0, 0.0] and seen[3][1] > 0


def test_ttl_expiry_and_reentry():
    t = TrendRef(64, ttl=2, warmup=1)
    e1, e2 = (A, B_, 1, 0, 1000), (A, C_, 1, 0, 1000)
    t.window(rows_of(e1, e2), NOOB)                                  # w1: both new
    t.window(rows_of(e2), NOOB)                                      # w2: e1 unseen, 2 - 1 < 2: kept
    assert len(t.entries) == 2 and t.stats["expired"] == 0
    t.window(rows_of(e2), NOOB)                                      # w3: 3 - 1 >= 2: e1 removed
    assert len(t.entries) == 1 and t.stats["expired"] == 1
    o = t.window(rows_of(e1, e2), NOOB)                              # w4: e1 is new again
    assert list(o["windows_seen"]) == [0, 3]
    assert t.entries["n"][0] == 1 and t.entries["last"][0] == 4
    t1 = TrendRef(64, ttl=1)
    t1.window(rows_of(e1, e2), NOOB); t1.window(rows_of(e2), NOOB)   # ttl 1: an entry lives only while it is seen
    assert len(t1.entries) == 1 and t1.stats["expired"] == 1


def test_alive_only_rows_neither_create_nor_refresh():
    t = TrendRef(64, warmup=1, ttl=2)
    o = t.window(rows_of((A, B_, 0, 0, 0)), NOOB)
    assert len(t.entries) == 0 and o["windows_seen"][0] == 0
    t.window(rows_of((A, B_, 1, 0, 4000)), NOOB)                     # w2: created
    o = t.window(rows_of((A, B_, 0, 0, 0)), NOOB)                    # w3: alive only — reported, not refreshed
    assert o["windows_seen"][0] == 1 and o["lat_dev"][0] == 0 and o["base_mean_us"][0] == np.float32(4.0)
    assert t.entries["n"][0] == 1 and t.entries["last"][0] == 2
    t.window(rows_of((A, B_, 0, 0, 0)), NOOB)                        # w4: 4 - 2 >= 2: expired although the edge is alive
    assert len(t.entries) == 0 and t.stats["expired"] == 1


def test_capacity_cut_in_key_order():
    t = TrendRef(64, max_entries=3, ttl=8)
    t.window(rows_of((A, ref(REF_KNOWN, 9), 1, 0, 10)), NOOB)        # one old entry
    edges = [(A, ref(REF_KNOWN, v), 1, 0, 10) for v in (2, 3, 4, 5, 9)]
    o = t.window(rows_of(*edges), NOOB)
    assert list(o["windows_seen"]) == [0, 0, 0, 0, 1]
    # kept: the old one; room 2: the first two new keys (to 2, 3) go in, 4 and 5 are dropped
    assert [int(k) & 0xFFFFFFFF for k in t.entries["to_key"]] == [2, 3, 9]
    assert t.stats == dict(windows=2, entries=3, inserted=3, expired=0, dropped=2)
    o = t.window(rows_of(*edges), NOOB)
    assert list(o["windows_seen"]) == [1, 1, 0, 0, 2]                # dropped ones are unseen again


def test_reversed_direction_and_outbound_ip_keys():
    obips = np.array([0x0A000001, 0x0A000102, 0xC0A80001], dtype=np.uint32)   # ascending, as the window lists them
    rows = rows_of((A, ref(REF_LABEL, 0), 1, 0, 10), (A, ref(REF_OBIP, 1), 1, 0, 10), (B_, ref(REF_KNOWN, 1), 1, 0, 10),
                   (ref(REF_LABEL, 4), A, 1, 0, 10), (ref(REF_OBIP, 0), A, 1, 0, 10), (ref(REF_OBIP, 2), B_, 1, 0, 10))
    fk, tk = row_keys(rows, obips)
    assert list(tk[:3]) == [(1 << 32) | 0, (2 << 32) | 0x0A000102, 1]
    assert list(fk[3:]) == [(1 << 32) | 4, (2 << 32) | 0x0A000001, (2 << 32) | 0xC0A80001]
    assert strictly_ascending(fk, tk)                                # KNOWN < LABEL < OBIP, ids and addresses ascending
    assert not strictly_ascending(fk[::-1], tk[::-1])
    # the same edge in the next window, whose outbound-IP list differs: the key (the address) matches, not the rank
    t = TrendRef(64, warmup=1)
    t.window(rows, obips)
    ob2 = np.array([0x01010101, 0x0A000001, 0x0A000102, 0xC0A80001], dtype=np.uint32)
    rows2 = rows_of((A, ref(REF_OBIP, 2), 1, 0, 10), (ref(REF_OBIP, 1), A, 1, 0, 10))
    o = t.window(rows2, ob2)
    assert list(o["windows_seen"]) == [1, 1]
    assert int(ref_keys([ref(REF_OBIP, 3)], ob2)[0]) == (2 << 32) | 0xC0A80001


trend_plan = plan_fixture("trend")


def _p(me, slots=1, ss=40, shift=0, warmup=0, ttl=0, maxe=0, lf=0, ef=0, res=0):
    return (me, slots, ss, shift, warmup, ttl, maxe, lf, ef, res)


SIZES = [1, 2, 255, 2047, 2048, 4096, 1 << 15, 1 << 18, (1 << 20) - 1, 1 << 20, 2_000_000, 1 << 22, 1 << 24]


def test_plan_sizes_fit_every_window(trend_plan):
    lines = [_p(me, slots) for me in SIZES for slots in (1, 2, 8)] + [_p(me, 1, maxe=m) for me in SIZES for m in (1, 2, 7, 33, 1 << 20)]
    for r in trend_plan(lines):
        assert r["rc"] == 0 and r["params_size"] == 40 and r["edge_trend_size"] == 16 and r["entry_size"] == 56
        me, C_ = r["max_edges"], r["entries"]
        assert C_ == r["max_entries"] >= 1
        assert 1 <= r["wgs"] <= r["max_wgs"] == 1024
        assert r["soa_bytes"] >= 56 * C_ and r["soa_bytes"] % 256 == 0
        assert r["rows_bytes"] >= 16 * me                              # every row of every window a slot can close
        assert r["blk_bytes"] >= 16 * r["wgs"] and r["thread_bytes"] >= 16 * 256 * r["wgs"] and r["ctl_bytes"] >= 64
        assert r["total_bytes"] == 2 * r["soa_bytes"] + r["ctl_bytes"] + r["blk_bytes"] + r["thread_bytes"] + r["slots"] * r["rows_bytes"]
        check_layout(r, {"soa0": 56 * C_, "soa1": 56 * C_, "ctl": 64, "blk": 16 * r["wgs"], "thread": 16 * 256 * r["wgs"], "rows": 16 * me}, per_slot=("rows",))
        check_soa(r)
        # the merge of B <= max_entries entries and E <= max_edges rows in spans of about eight per thread, below the workgroup cap
        if r["wgs"] < 1024:
            assert r["wgs"] * 256 * r["per_thread"] >= C_ + me
    c3 = {(r["max_edges"], r["slots"]): r for r in trend_plan([_p(1 << 20)])}[(1 << 20, 1)]
    assert c3["entries"] == 2 << 20 and c3["wgs"] == 1024 and c3["total_bytes"] < 260 << 20


def test_plan_defaults_and_invalid_parameters(trend_plan):
    d, = trend_plan([_p(1000)])
    assert (d["shift"], d["warmup"], d["ttl"], d["max_entries"], d["lat_floor_ns"], d["err_floor"]) == (4, 4, 64, 2000, 1000, 10486)
    k, = trend_plan([_p(1000, shift=10, warmup=1, ttl=1, maxe=5, lf=7, ef=9)])
    assert (k["shift"], k["warmup"], k["ttl"], k["max_entries"], k["lat_floor_ns"], k["err_floor"]) == (10, 1, 1, 5, 7, 9)
    bad = trend_plan([_p(1000, shift=11), _p(1000, ss=36), _p(1000, ss=48), _p(1000, res=1), _p(1000, maxe=(1 << 31) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
    ok, = trend_plan([_p(1000, maxe=1 << 31)])
    assert ok["rc"] == 0
