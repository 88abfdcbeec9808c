"""CPU tests of K8's vanished list and of the selection by a trend key: the numpy reference tests/vanish_ref.py against hand-computed
sequences, the Python dtypes and constants against include/servicegraph.h, and the plan in alaz_amd/csrc/sg_plan.hpp
(tests/micro/plan_driver.cpp, stage vanish) — parameter checks and defaults, and memory for every window slot."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.helpers import ref
from tests.host_scaffold import trend_rows_of as rows_of
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.select_by_ref import ref_select_by
from tests.trend_ref import REF_KNOWN, TrendRef
from tests.vanish_ref import NO_ROW, VanishRef

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOOB = np.zeros(0, np.uint32)

A, B_, C_, D_ = (ref(REF_KNOWN, v) for v in (1, 2, 3, 4))
AB, AC, AD = (A, B_, 1, 0, 1000), (A, C_, 1, 0, 2000), (A, D_, 1, 0, 3000)


def to_of(v):
    return [int(k) & 0xFFFFFFFF for k in v["to_key"]]


def test_dtypes_and_constants_match_the_header():
    assert engine.VANISHED_DTYPE.itemsize == 64 and C.sizeof(engine.SgVanishedParams) == 16
    f = engine.VANISHED_DTYPE.fields
    assert (f["lat_mean"][1], f["err_dev"][1], f["n"][1], f["last"][1], f["row"][1], f["reserved"][1]) == (16, 40, 48, 52, 56, 60)
    assert engine.SgVanishedParams.max_rows.offset == 12
    h = open(os.path.join(ROOT, "include", "servicegraph.h")).read()
    sel = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define SG_SEL_([A-Z_]+)\s+(\d+)u", h)}
    assert sel == engine.SEL_BY


def test_silent_one_reports_each_silence_once():
    t = TrendRef(64, warmup=1, ttl=8)
    v = VanishRef(t, silent_windows=1)
    _, l, n = v.window(rows_of(AB, AC), NOOB)                          # w1: both new, nothing old
    assert n == 0 and len(l) == 0
    _, l, n = v.window(rows_of(AC), NOOB)                              # w2: A->B silent for one window
    assert n == 1 and to_of(l) == [2] and l["row"][0] == NO_ROW
    assert (l["n"][0], l["last"][0], l["lat_mean"][0]) == (1, 1, 1000.0)
    _, l, n = v.window(rows_of(AC), NOOB)                              # w3: still silent, 3 - 1 = 2: not again
    assert n == 0
    v.window(rows_of(AB, AC), NOOB)                                    # w4: back
    _, l, n = v.window(rows_of(AC), NOOB)                              # w5: silent again: reported again
    assert n == 1 and to_of(l) == [2] and (l["n"][0], l["last"][0]) == (2, 4)


def test_silent_three_min_seen_and_the_alive_only_row():
    t = TrendRef(64, warmup=2, ttl=8)
    v = VanishRef(t, silent_windows=3)                                 # min_seen = the trend's warmup = 2
    v.window(rows_of(AB, AC, AD), NOOB)                                # w1
    v.window(rows_of(AB, AC), NOOB)                                    # w2: A->D seen once only
    counts = []
    for _ in range(3):                                                 # w3..w5: A->B alive-only, A->C and A->D absent
        _, l, n = v.window(rows_of((A, B_, 0, 0, 0)), NOOB)
        counts.append(n)
    assert counts == [0, 0, 2]                                         # w5 - last(2) == 3: A->B and A->C; A->D has n = 1 < 2
    assert to_of(l) == [2, 3] and list(l["row"]) == [0, NO_ROW]
    t2 = TrendRef(64, warmup=2, ttl=8)
    v2 = VanishRef(t2, silent_windows=3, min_seen=1)
    for rows in (rows_of(AB, AC, AD), rows_of(AB, AC), rows_of(), rows_of()):
        v2.window(rows, NOOB)
    _, l, n = v2.window(rows_of(), NOOB)                               # w5: A->B, A->C (last 2); A->D (last 1) came at w4
    assert n == 2 and to_of(l) == [2, 3]


def test_dropped_entries_are_never_reported_and_max_rows_cuts_in_key_order():
    t = TrendRef(64, warmup=1, ttl=8, max_entries=2)
    v = VanishRef(t, silent_windows=1, max_rows=1)
    v.window(rows_of(AB, AC, AD), NOOB)                                # capacity 2: A->D dropped
    _, l, n = v.window(rows_of(), NOOB)
    assert n == 2 and to_of(l) == [2]                                  # A->B and A->C vanished; max_rows 1 keeps the first key
    t2 = TrendRef(64, warmup=1, ttl=2)
    v2 = VanishRef(t2, silent_windows=1)
    v2.window(rows_of(AB), NOOB)
    _, l, n = v2.window(rows_of(), NOOB)                               # reported at w2 ...
    assert n == 1
    _, l, n = v2.window(rows_of(), NOOB)                               # ... expired at w3 (ttl 2), never reported again
    assert n == 0 and len(t2.entries) == 0
    with pytest.raises(AssertionError):
        VanishRef(TrendRef(64, ttl=2), silent_windows=2)               # silent_windows < ttl


def test_selection_keys_by_trend_value():
    """the semantics tests/test_gpu_select_by.py checks the engine against: a plain float comparison and k7's order"""
    tr = np.zeros(6, dtype=engine.TREND_DTYPE)
    tr["lat_dev"] = [1.5, np.nan, -0.0, 0.0, 3.0, 1.5]
    tr["windows_seen"] = [0, 0, 3, 0, 1, 0]
    rows = np.zeros(6, dtype=EDGE_OUT_DTYPE)
    rows["count"] = [1, 1, 1, 0, 1, 2]
    assert list(ref_select_by(rows, tr, "lat_dev", 0, 0.0)) == [0, 2, 3, 4, 5]          # NaN never, -0.0 >= 0.0
    assert list(ref_select_by(rows, tr, "lat_dev", 3, float("-inf"))) == [4, 0, 5]
    assert list(ref_select_by(rows, tr, "lat_dev", 5, float("-inf"))) == [4, 0, 5, 2, 3]  # -0.0 == +0.0: by position
    assert list(ref_select_by(rows, tr, "new", 0, 99.0)) == [0, 1, 5]                    # min_value ignored
    assert list(ref_select_by(rows, tr, "new", 2, 0.0)) == [0, 1]


vanish_plan = plan_fixture("vanish")


def _p(me, slots=1, warmup=0, ttl=0, maxe=0, ss=16, silent=0, seen=0, rows=0):
    return (me, slots, warmup, ttl, maxe, ss, silent, seen, rows)


def test_plan_defaults_and_invalid_parameters(vanish_plan):
    d, = vanish_plan([_p(1000)])
    assert d["rc"] == 0 and d["params_size"] == 16 and d["vanished_size"] == 64
    assert (d["silent_windows"], d["min_seen"], d["max_rows"]) == (1, 4, 2000)      # max_rows: min(65536, max_entries = 2 x 1000)
    big, = vanish_plan([_p(1 << 20)])
    assert big["max_rows"] == 65536
    k, = vanish_plan([_p(1000, warmup=7, ttl=5, silent=4, seen=2, rows=9)])
    assert (k["silent_windows"], k["min_seen"], k["max_rows"]) == (4, 2, 9)
    w, = vanish_plan([_p(1000, warmup=7)])
    assert w["min_seen"] == 7
    bad = vanish_plan([_p(1000, ttl=5, silent=5), _p(1000, ttl=5, silent=9), _p(1000, ttl=1), _p(1000, ss=12), _p(1000, ss=20),
                       _p(1000, maxe=10, rows=11)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 6
    ok, = vanish_plan([_p(1000, maxe=10, rows=10, ttl=2, silent=1)])
    assert ok["rc"] == 0


SIZES = [1, 2, 255, 2048, 1 << 15, 1 << 20, 2_000_000, 1 << 24]


def test_plan_memory_for_every_slot(vanish_plan):
    lines = [_p(me, slots) for me in SIZES for slots in (1, 2, 8)] + [_p(me, 3, maxe=m, rows=r) for me in SIZES for m, r in ((7, 7), (1 << 20, 1))]
    for r in vanish_plan(lines):
        assert r["rc"] == 0 and r["rows"] == r["max_rows"] >= 1
        assert r["list_bytes"] >= 64 * r["max_rows"] and r["list_bytes"] % 256 == 0 and r["count_bytes"] >= 8
        assert r["thread_bytes"] >= 4 * r["threads"] * r["wgs"] and r["blk_bytes"] >= 4 * r["wgs"]
        assert r["total_bytes"] == r["thread_bytes"] + r["blk_bytes"] + r["slots"] * (r["list_bytes"] + r["count_bytes"])
        check_layout(r, {"thread": 4 * r["threads"] * r["wgs"], "blk": 4 * r["wgs"], "list": 64 * r["max_rows"], "count": 8}, per_slot=("list", "count"))
