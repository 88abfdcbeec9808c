"""CPU tests of the traffic baselines (K23): the numpy references of tests/traffic_ref.py against a second formulation written apart
from them (a dict keyed by (from_key, to_key), plain Python floats, one sample at a time), against hand-computed answers, the
scenario the stage is for — a drop of traffic that latency and error ratio do not see — the plan in alaz_amd/csrc/sg_plan.hpp
(tests/micro/plan_driver.cpp, stage traffic_trend) and the header's constants against alaz_amd/engine.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.engine import EDGE_OUT_DTYPE, GROUP_EDGE_DTYPE, NODE_DTYPE, NO_GROUP as NO, REF_GROUP
from tests.group_nodes_ref import GroupNodeTrendRef, group_nodes_ref
from tests.group_ref import group_ref
from tests.group_trend_ref import group_keys, workload_keys
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests.traces import _random_map, _random_rows
from tests.traffic_ref import (EdgeTrafficRef, GroupTrafficRef, NodeTrafficRef, WorkloadTrafficRef, ref_select_traffic,
                               traffic_column)
from tests.trend_ref import ref_keys, row_keys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U32_MAX = 0xFFFFFFFF
G = lambda g: (REF_GROUP << 30) | g                                   # noqa: E731  a group ref


# ---- the second formulation -------------------------------------------------------------------------------------------------------
class DictTraffic:
    """one baseline as a dict: key -> [rate_mean, rate_dev, load_mean, load_dev, n, last].  window(samples) takes the window's
    samples (key, count, sum_ns) in key order and returns their (rate_dev, load_dev, base, seen)"""

    def __init__(self, cap, shift, warmup, ttl, rate_floor, load_floor_ns):
        self.cap, self.alpha, self.warmup, self.ttl = cap, 2.0 ** -shift, warmup, ttl
        self.rate_floor, self.load_floor = 1000.0 * rate_floor, float(load_floor_ns)
        self.d, self.w = {}, 0
        self.stats = dict(windows=0, entries=0, inserted=0, expired=0, dropped=0)

    def window(self, samples):
        self.w += 1
        out, updates, fresh = [], [], []
        for key, c, s in samples:
            e = self.d.get(key)
            xr, xl = 1000.0 * float(min(int(c), 1 << 42)), float(min(int(s), 1 << 52))
            rd = ld = base = np.float32(0.0)
            seen = 0
            if e is not None:
                seen, base = e[4], np.float32(e[0] / 1000.0)
                if c > 0 and seen >= self.warmup:
                    rd = np.float32((xr - e[0]) / (e[1] if e[1] > self.rate_floor else self.rate_floor))
                    ld = np.float32((xl - e[2]) / (e[3] if e[3] > self.load_floor else self.load_floor))
            out.append((rd, ld, base, seen))
            if c > 0:
                (updates if e is not None else fresh).append((key, xr, xl))
        touched = set()
        for key, xr, xl in updates:                                   # after every row was scored: from the entries as they stood
            e = self.d[key]
            dr, dl = xr - e[0], xl - e[2]
            e[0] = e[0] + dr * self.alpha; e[1] = e[1] + (abs(dr) - e[1]) * self.alpha
            e[2] = e[2] + dl * self.alpha; e[3] = e[3] + (abs(dl) - e[3]) * self.alpha
            e[4] = min(e[4] + 1, U32_MAX); e[5] = self.w
            touched.add(key)
        for key in [k for k, e in self.d.items() if k not in touched and self.w - e[5] >= self.ttl]:
            del self.d[key]; self.stats["expired"] += 1
        room = max(self.cap - len(self.d), 0)
        for key, xr, xl in sorted(fresh)[:room]:
            self.d[key] = [xr, 0.0, xl, 0.0, 1, self.w]
        s = self.stats
        s["windows"] += 1; s["entries"] = len(self.d); s["inserted"] += min(len(fresh), room); s["dropped"] += len(fresh) - min(len(fresh), room)
        return out

    def entries(self):
        return [(k[0], k[1], *self.d[k]) for k in sorted(self.d)]


def _entries_of(ref):
    e = ref.entries
    return [(int(a), int(b), float(c), float(d), float(f), float(g), int(h), int(i)) for a, b, c, d, f, g, h, i in
            zip(e["from_key"], e["to_key"], e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"])]


def _node_samples(nodes, keys):
    out = []
    for k in range(len(nodes)):
        out.append(((int(keys[k]), 0), int(nodes["in_count"][k]), int(nodes["in_sum_ns"][k])))
        out.append(((int(keys[k]), 1), int(nodes["out_count"][k]), int(nodes["out_sum_ns"][k])))
    return out


def _edge_samples(rows, fk, tk):
    return [((int(fk[j]), int(tk[j])), int(rows["count"][j]), int(rows["sum_ns"][j])) for j in range(len(rows))]


def _node_rows(out):
    got = np.zeros(len(out) // 2, dtype=engine.NODE_TREND_DTYPE)
    for j, (rd, ld, base, seen) in enumerate(out):
        s = "in" if j % 2 == 0 else "out"
        got[f"{s}_lat_dev"][j // 2], got[f"{s}_err_dev"][j // 2], got[f"{s}_base_mean_us"][j // 2], got[f"{s}_seen"][j // 2] = rd, ld, base, seen
    return got


def _edge_rows(out):
    got = np.zeros(len(out), dtype=engine.TREND_DTYPE)
    for j, (rd, ld, base, seen) in enumerate(out):
        got["lat_dev"][j], got["err_dev"][j], got["base_mean_us"][j], got["windows_seen"][j] = rd, ld, base, seen
    return got


@pytest.mark.parametrize("block", range(8))
def test_references_against_the_dict_formulation(block):
    """40 seeds a block: chains of 6 - 10 windows of random rows under maps that group nothing, something and everything; every
    window's traffic rows, and the baseline and the statistics after it, in all four spaces"""
    for seed in range(40 * block, 40 * block + 40):
        rng = np.random.default_rng(23000 + seed)
        mk, ml = int(rng.integers(41, 80)), int(rng.integers(1, 8))      # (_random_rows makes pods of ids below 40 whatever mk is)
        mg = int(rng.integers(1, mk + 1))
        gmap = (np.full(mk, NO, np.uint32), _random_map(rng, mk, mg), np.zeros(mk, np.uint32))[seed % 3]
        p = dict(shift=int(rng.integers(1, 5)), warmup=int(rng.integers(1, 4)), ttl=int(rng.integers(1, 5)), max_entries=int(rng.integers(3, 80)))
        fl = dict(rate_floor=int(rng.integers(1, 1 << 20)), load_floor_ns=int(rng.integers(1, 1 << 52)))
        ncap, nc = mk + ml + 40, mg + mk + ml + 40
        refs = EdgeTrafficRef(1 << 12, **p, **fl), NodeTrafficRef(ncap, **p, **fl), GroupTrafficRef(1 << 12, **p, **fl), WorkloadTrafficRef(nc, **p, **fl)
        dicts = [DictTraffic(p["max_entries"], p["shift"], p["warmup"], p["ttl"], **fl) for _ in range(4)]
        for w in range(int(rng.integers(6, 11))):
            rows = _random_rows(rng, mk, ml, int(rng.integers(0, 120)))
            obips = np.sort(rng.choice(1 << 24, 40, replace=False)).astype(np.uint32) + np.uint32(1 << 24)
            nodes = nodes_ref(rows)
            ge, _, _ = group_ref(rows, gmap, mg, mk, ml)
            gn = group_nodes_ref(ge, mg, mk, ml)
            want = refs[0].window(rows, obips)
            assert _edge_rows(dicts[0].window(_edge_samples(rows, *row_keys(rows, obips)))).tobytes() == want.tobytes(), (seed, w)
            want = refs[1].window(nodes, obips)
            assert _node_rows(dicts[1].window(_node_samples(nodes, ref_keys(nodes["ref"], obips)))).tobytes() == want.tobytes(), (seed, w)
            want = refs[2].window(ge, obips)
            assert _edge_rows(dicts[2].window(_edge_samples(ge, *group_keys(ge, obips)))).tobytes() == want.tobytes(), (seed, w)
            want = refs[3].window(gn, obips)
            assert _node_rows(dicts[3].window(_node_samples(gn, workload_keys(gn["ref"], obips)))).tobytes() == want.tobytes(), (seed, w)
            for r, d in zip(refs, dicts):
                assert _entries_of(r) == d.entries() and r.stats == d.stats, (seed, w)


# ---- hand-computed answers ----------------------------------------------------------------------------------------------------------
def _ge(edges):
    """group edges (from group, to group, count, sum_ns), ascending"""
    g = np.zeros(len(edges), dtype=GROUP_EDGE_DTYPE)
    for i, (f, t, c, s) in enumerate(edges):
        g["from_ref"][i], g["to_ref"][i], g["count"][i], g["sum_ns"][i] = G(f), G(t), c, s
    return g


def _entry(ref, f, t):
    e = ref.entries
    return e[(e["from_key"] == f) & (e["to_key"] == t)]


def _row(t):
    return tuple(float(t[f]) for f in ("lat_dev", "err_dev", "base_mean_us")) + (int(t["windows_seen"]),)


def test_one_edge_by_hand_warmup_a_halving_a_doubling_expiry_and_the_capacity_cut():
    """workload edge 3 -> 5 with alpha = 1/2, warmup 2, ttl 2, two entries at most, floors of 16 requests and 1 ms of busy time:
    64 requests of 1 ms a window"""
    ms = 1_000_000
    ref = GroupTrafficRef(100, shift=1, warmup=2, ttl=2, max_entries=2, rate_floor=16, load_floor_ns=ms)
    ob = np.zeros(0, np.uint32)
    X = _ge([(3, 5, 64, 64 * ms)])
    assert _row(ref.window(X, ob)[0]) == (0, 0, 0, 0)                 # w1: a new entry; the row is zero
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (64_000.0, 0.0, 64.0 * ms, 0.0, 1, 1)
    assert _row(ref.window(X, ob)[0]) == (0, 0, 64.0, 1)              # w2: seen 1 < warmup: the baseline rate only, in requests
    # w3: a halving — 32 requests, the same latency: (32000 - 64000) / max(0, 16 * 1000), (32 ms - 64 ms) / max(0, 1 ms)
    assert _row(ref.window(_ge([(3, 5, 32, 32 * ms)]), ob)[0]) == (-2.0, -32.0, 64.0, 2)
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (48_000.0, 16_000.0, 48.0 * ms, 16.0 * ms, 3, 3)
    # w4: a doubling of the first rate — 128 requests: (128000 - 48000) / 16000 = 5, the load likewise
    assert _row(ref.window(_ge([(3, 5, 128, 128 * ms)]), ob)[0]) == (5.0, 5.0, 48.0, 3)
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (88_000.0, 48_000.0, 88.0 * ms, 48.0 * ms, 4, 4)
    O = _ge([(4, 4, 1, 7)])
    ref.window(O, ob)                                                 # w5: X silent for one window: kept
    assert len(_entry(ref, 3, 5)) == 1 and ref.stats["entries"] == 2
    alive = ref.window(_ge([(3, 5, 0, 0), (4, 4, 1, 7)]), ob)[0]      # w6: a sample with c == 0 neither scores nor refreshes: 6 - 4 = ttl, expired
    assert _row(alive) == (0, 0, 88.0, 4)
    assert len(_entry(ref, 3, 5)) == 0 and ref.stats["expired"] == 1 and ref.stats["entries"] == 1
    # w7: three new keys beside the kept one: room for the first in key order only
    ref.window(_ge([(3, 5, 2, 9), (4, 4, 1, 7), (6, 1, 1, 1), (9, 9, 1, 1)]), ob)
    assert [(int(a), int(b)) for a, b in zip(ref.entries["from_key"], ref.entries["to_key"])] == [(3, 5), (4, 4)]
    assert ref.stats == dict(windows=7, entries=2, inserted=3, expired=1, dropped=2)
    assert _entry(ref, 3, 5)[0]["lat_mean"] == 2000.0 and _entry(ref, 3, 5)[0]["err_mean"] == 9.0 and _entry(ref, 3, 5)[0]["n"] == 1


def _node_row(ref, in_c=0, in_sum=0, out_c=0, out_sum=0, in_err=0):
    n = np.zeros(1, dtype=NODE_DTYPE)
    n["ref"], n["in_count"], n["in_sum_ns"], n["in_err"], n["out_count"], n["out_sum_ns"] = ref, in_c, in_sum, in_err, out_c, out_sum
    return n


def test_the_side_mapping_and_a_silent_side_beside_a_live_one():
    """a node called 40 times and calling 5 times: (key, 0) is the IN side, (key, 1) the OUT side; then its out side falls silent
    (c == 0) while the in side goes on: the out entry is neither refreshed nor scored, the in side is"""
    ob = np.zeros(0, np.uint32)
    for Ref, key in ((NodeTrafficRef, 7), (WorkloadTrafficRef, (1 << 32) + 7)):
        ref = Ref(16, shift=1, warmup=1, rate_floor=1, load_floor_ns=1)
        both = _node_row(7, in_c=40, in_sum=4000, out_c=5, out_sum=900)
        ref.window(both, ob)
        e = ref.entries
        assert e["from_key"].tolist() == [key, key] and e["to_key"].tolist() == [0, 1]
        assert e["lat_mean"].tolist() == [40_000.0, 5_000.0] and e["err_mean"].tolist() == [4000.0, 900.0]
        t = ref.window(_node_row(7, in_c=20, in_sum=4000, out_c=0, out_sum=0), ob)[0]
        assert (t["in_lat_dev"], t["in_err_dev"], t["in_base_mean_us"], t["in_seen"]) == (-20.0, 0.0, 40.0, 1)     # (20000 - 40000) / 1000
        assert (t["out_lat_dev"], t["out_err_dev"], t["out_base_mean_us"], t["out_seen"]) == (0.0, 0.0, 5.0, 1)    # silent: the base and seen only
        e = ref.entries
        assert e["n"].tolist() == [2, 1] and e["last"].tolist() == [2, 1] and e["lat_mean"].tolist() == [30_000.0, 5_000.0]
    # a node that only calls and one that is only called: one entry each, on its own side
    ref = NodeTrafficRef(16, shift=1, warmup=1, rate_floor=1, load_floor_ns=1)
    ref.window(np.concatenate([_node_row(3, out_c=2, out_sum=10), _node_row(4, in_c=2, in_sum=10)]), ob)
    assert [(int(a), int(b)) for a, b in zip(ref.entries["from_key"], ref.entries["to_key"])] == [(3, 1), (4, 0)]


def test_both_clamps():
    """c > 2^42 and sum_ns > 2^52 (no engine window reaches either): the samples stop at 1000 * 2^42 and 2^52, both exact"""
    ob = np.zeros(0, np.uint32)
    ref = GroupTrafficRef(100, shift=1, warmup=1, rate_floor=1, load_floor_ns=1)
    ref.window(_ge([(1, 2, (1 << 42) + 5, (1 << 52) + 12345), (1, 3, 1 << 42, 1 << 52), (1, 4, (1 << 42) - 1, (1 << 52) - 1)]), ob)
    e = ref.entries
    assert e["lat_mean"].tolist() == [1000.0 * (1 << 42), 1000.0 * (1 << 42), 1000.0 * ((1 << 42) - 1)]
    assert e["err_mean"].tolist() == [float(1 << 52), float(1 << 52), float((1 << 52) - 1)]
    assert all(float(x).is_integer() and x < 2.0 ** 53 for x in e["lat_mean"])
    t = ref.window(_ge([(1, 2, 1 << 63, (1 << 64) - 1)]), ob)[0]      # far past both: the same sample, no deviation
    assert _row(t) == (0.0, 0.0, float(np.float32(1 << 42)), 1)
    w = NodeTrafficRef(8, shift=1, warmup=1, rate_floor=1, load_floor_ns=1)
    w.window(_node_row(9, in_c=(1 << 42) + 1, in_sum=(1 << 52) + 1, out_c=1 << 50, out_sum=1 << 60), ob)
    assert w.entries["lat_mean"].tolist() == [1000.0 * (1 << 42)] * 2 and w.entries["err_mean"].tolist() == [float(1 << 52)] * 2


def test_how_the_floor_defaults_resolve():
    """rate_floor 0 = 8 requests, load_floor_ns 0 = 1 000 000: the walk's floors are 8000.0 and 1e6 — the only test on the defaults"""
    ob = np.zeros(0, np.uint32)
    for kw in (dict(), dict(rate_floor=0, load_floor_ns=0), dict(rate_floor=8, load_floor_ns=1_000_000)):
        ref = GroupTrafficRef(100, shift=1, warmup=1, **kw)
        assert (ref.lat_floor, ref.err_floor) == (8000.0, 1_000_000.0)
        ref.window(_ge([(1, 2, 100, 50_000_000)]), ob)
        t = ref.window(_ge([(1, 2, 84, 47_000_000)]), ob)[0]          # dev 0: both floors decide
        assert _row(t) == (-2.0, -3.0, 100.0, 1)                      # (84000 - 100000) / 8000, (47e6 - 50e6) / 1e6
    assert engine.TRAFFIC_DEFAULTS["rate_floor"] == 8 and engine.TRAFFIC_DEFAULTS["load_floor_ns"] == 1_000_000
    for Ref, cap in ((EdgeTrafficRef, 2 * 500), (GroupTrafficRef, 2 * 500), (NodeTrafficRef, 4 * 500), (WorkloadTrafficRef, 4 * 500)):
        assert Ref(500).cap == cap                                    # max_entries 0: the mean baseline's default of the space


def test_the_selection_reference_over_the_signed_column():
    t = np.zeros(6, dtype=engine.NODE_TREND_DTYPE)
    t["in_lat_dev"] = [2.0, -5.0, 0.0, -0.0, np.nan, -1.0]
    t["out_err_dev"] = [-3.0, -2.0, -1.0, -4.0, -0.5, -6.0]
    assert traffic_column(t, "drop", "in").view(np.uint32).tolist() == (t["in_lat_dev"].view(np.uint32) ^ np.uint32(1 << 31)).tolist()
    assert ref_select_traffic(t, "surge", "in", 0, -np.inf).tolist() == [0, 1, 2, 3, 5]           # NaN never
    assert ref_select_traffic(t, "surge", "in", 3, -np.inf).tolist() == [0, 2, 3]                 # +0.0 == -0.0: by position
    assert ref_select_traffic(t, "drop", "in", 3, -np.inf).tolist() == [1, 5, 2]                  # -(-5), -(-1), then the zeros by position
    assert ref_select_traffic(t, "drop", "in", 0, 0.5).tolist() == [1, 5]                         # min_value on the signed value
    assert ref_select_traffic(t, "load_up", "out", 1, 0.0).tolist() == []                         # every deviation negative: nothing surges
    assert ref_select_traffic(t, "load_down", "out", 0, 0.0).tolist() == [0, 1, 2, 3, 4, 5]       # and everything drops
    assert ref_select_traffic(t, "load_down", "out", 2, 0.0).tolist() == [5, 3]
    e = np.zeros(3, dtype=engine.TREND_DTYPE); e["lat_dev"] = [1.0, -2.0, 3.0]
    assert ref_select_traffic(e, "drop", None, 1, -np.inf).tolist() == [1]


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------
def _workloads(counts, lat_ns, err_ppm):
    n = np.zeros(len(counts), dtype=NODE_DTYPE)
    for i, (c, l, e) in enumerate(zip(counts, lat_ns, err_ppm)):
        n["ref"][i], n["in_count"][i], n["in_sum_ns"][i], n["in_err"][i] = G(i), c, c * l, c * e // 1_000_000
    return n


def scenario():
    """Four workloads, about 1000 requests a window each, +-5 %; each request about 2 ms, +-5 %; one request in a hundred fails,
    +-20 % of that.  In window 30 an upstream failure cuts workload 2's inbound traffic to a tenth; the requests that still arrive
    take 2 ms and fail at 1 %.  Returns (the calm windows' |lat_dev|, |err_dev| of the mean baseline and |rate_dev| of the traffic
    baseline for workload 2, the last window's mean-baseline row, its traffic row, the traffic rows of that window)"""
    rng = np.random.default_rng(23)
    p = dict(shift=3, warmup=4)
    traffic, mean = WorkloadTrafficRef(16, rate_floor=8, load_floor_ns=1_000_000, **p), GroupNodeTrendRef(16, **p)
    ob = np.zeros(0, np.uint32)
    calm = dict(lat=[], err=[], rate=[])
    for w in range(31):
        counts = [int(c) for c in rng.integers(950, 1051, 4)]
        lat = [int(x) for x in rng.integers(1_900_000, 2_100_001, 4)]
        err = [int(x) for x in rng.integers(8_000, 12_001, 4)]
        if w == 30:
            counts[2], lat[2], err[2] = 100, 2_000_000, 10_000
        rows = _workloads(counts, lat, err)
        t, m = traffic.window(rows, ob), mean.window(rows, ob)
        if 8 <= w < 30:
            calm["lat"].append(abs(float(m["in_lat_dev"][2]))); calm["err"].append(abs(float(m["in_err_dev"][2])))
            calm["rate"].append(abs(float(t["in_lat_dev"][2])))
    return calm, m[2], t[2], t


def test_a_drop_of_traffic_that_latency_and_error_ratio_do_not_see():
    calm, m, t, rows = scenario()
    band_lat, band_err, band_rate = max(calm["lat"]), max(calm["err"]), max(calm["rate"])
    assert 0 < band_lat < 4 and 0 < band_err < 4 and 0 < band_rate < 4           # calm windows stay within a few deviations
    assert abs(float(m["in_lat_dev"])) <= band_lat and abs(float(m["in_err_dev"])) <= band_err   # the mean baseline stays inside its calm band
    rate_dev, load_dev = float(t["in_lat_dev"]), float(t["in_err_dev"])
    assert rate_dev < -10 * band_rate and load_dev < -10                          # the rate falls far outside it, and the load with it
    assert t["in_base_mean_us"] == pytest.approx(1000.0, rel=0.05)                # the baseline reads as requests per window
    assert ref_select_traffic(rows, "drop", "in", 1, -np.inf).tolist() == [2]
    assert ref_select_traffic(rows, "drop", "in", 0, 10.0).tolist() == [2]        # and alone past ten deviations
    assert ref_select_traffic(rows, "surge", "in", 0, 10.0).tolist() == []
    # the two values DESIGN §3 K23 quotes
    assert (round(float(m["in_lat_dev"]), 2), round(rate_dev, 1)) == SCENARIO_DESIGN_VALUES


SCENARIO_DESIGN_VALUES = (-0.13, -26.0)                                  # (the mean baseline's lat_dev, the traffic baseline's rate_dev)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("traffic_trend")


def _p(spaces=15, on=15, me=4096, ncap=1000, nc=1500, slots=1, ss=40, shift=0, warmup=0, ttl=0, maxe=0, lf=0, rf=0, res=0):
    return (spaces, on, me, ncap, nc, slots, ss, shift, warmup, ttl, maxe, lf, rf, res)


def test_plan_is_the_mean_baselines_plan_per_space_in_64_bits(plan):
    cases = [_p(ncap=n, me=me, nc=nc, slots=s) for n, me, nc in ((1, 1, 1), (300, 1 << 15, 700), (70_000, 1_250_000, 140_000), (1 << 21, 1 << 31, 1 << 21))
             for s in (1, 3)] + [_p(maxe=m) for m in (1, 7, 1 << 20)]
    for r in plan(cases):
        assert r["rc"] == 0 and r["spaces"] == 15 and r["node_trend_size"] == 32 and r["trend_size"] == 16 and r["params_size"] == 40
        n, me, nc = r["ncap"], r["max_edges"], r["nc"]
        for k, (samples, rows, row) in enumerate(((me, me, 16), (2 * n, n, 32), (me, me, 16), (2 * nc, nc, 32))):
            t = r["sp"][k]
            cap = t["entries"]
            assert cap == t["max_entries"] >= 1 and 1 <= t["wgs"] <= 1024
            assert t["total_bytes"] == 2 * t["soa_bytes"] + t["ctl_bytes"] + t["blk_bytes"] + t["thread_bytes"] + t["slots"] * t["rows_bytes"]
            check_layout(t, {"soa0": 56 * cap, "soa1": 56 * cap, "ctl": 64, "blk": 16 * t["wgs"], "thread": 16 * 256 * t["wgs"], "rows": row * rows},
                         per_slot=("rows",))
            check_soa(t)
            if t["wgs"] < 1024:
                assert t["wgs"] * 256 * t["per_thread"] >= cap + samples
        assert r["total_bytes"] == sum(t["total_bytes"] for t in r["sp"])
        assert r["sp"][0] == r["sp"][2]                               # the two edge-shaped spaces: one rule
    big, = plan([_p(ncap=1 << 21, me=1 << 31, nc=1 << 21)])
    for k in (0, 2):
        g = big["sp"][k]
        assert g["entries"] == 1 << 31 and g["rows_bytes"] == 16 << 31 and g["soa_bytes"] >= 56 << 31 and g["total_bytes"] > 1 << 37    # past 2^32
    assert big["sp"][1]["entries"] == 4 << 21 and big["sp"][3]["entries"] == 4 << 21


def test_plan_defaults_floors_and_what_is_refused(plan):
    d, = plan([_p(me=4096, ncap=1000, nc=1500)])
    assert [t["max_entries"] for t in d["sp"]] == [8192, 4000, 8192, 6000]   # plan_trend's rule, plan_node_trend's, plan_group_trend's, the workloads'
    assert all((t["shift"], t["warmup"], t["ttl"]) == (4, 4, 64) for t in d["sp"])
    assert (d["rate_floor"], d["load_floor_ns"], d["lat_floor"], d["err_floor"]) == (8, 1_000_000, 8000.0, 1_000_000.0)
    f, = plan([_p(rf=U32_MAX, lf=1 << 52)])
    assert (f["rate_floor"], f["load_floor_ns"], f["lat_floor"], f["err_floor"]) == (U32_MAX, 1 << 52, 1000.0 * U32_MAX, float(1 << 52))
    one, = plan([_p(spaces=4, on=5)])
    assert one["spaces"] == 4 and [t is None for t in one["sp"]] == [True, True, False, True] and one["total_bytes"] == one["sp"][2]["total_bytes"]
    bad = plan([_p(spaces=0), _p(spaces=16), _p(spaces=31), _p(shift=11), _p(ss=36), _p(ss=32), _p(res=1), _p(maxe=(1 << 31) + 1), _p(lf=(1 << 52) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * len(bad)
    off = plan([_p(spaces=2, on=13), _p(spaces=15, on=3), _p(spaces=8, on=1)])
    assert [r["rc"] for r in off] == [engine.SG_ESTATE] * 3
    assert plan([_p(spaces=17, on=1)])[0]["rc"] == engine.SG_EINVAL   # unknown bits before the state


# ---- the header's constants --------------------------------------------------------------------------------------------------------------
def test_the_headers_constants_and_struct_are_the_front_ends(tmp_path):
    with open(os.path.join(ROOT, "include", "servicegraph.h")) as f:
        h = f.read()
    d = {n: int(v) for n, v in re.findall(r"#define\s+(SG_T(?:SEL)?_[A-Z_]+)\s+(\d+)u", h)}
    assert {n[5:].lower(): v for n, v in d.items() if n.startswith("SG_T_")} == engine.T_SPACES == dict(edges=1, nodes=2, groups=4, group_nodes=8)
    assert {n[8:].lower(): d[n] for n in ("SG_TSEL_SURGE", "SG_TSEL_DROP", "SG_TSEL_LOAD_UP", "SG_TSEL_LOAD_DOWN")} == engine.TSEL_BY
    assert {"in": d["SG_TSEL_IN"], "out": d["SG_TSEL_OUT"]} == engine.TSEL_SIDE
    assert len(d) == 10
    body = re.search(r"typedef struct sg_traffic_params \{(.*?)\} sg_traffic_params;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t)\s+(\w+);", body, re.M)
    ctype = dict(uint32_t=C.c_uint32, uint64_t=C.c_uint64)
    assert [(n, ctype[t]) for t, n in fields] == list(engine.TrafficParams._fields_)
    assert C.sizeof(engine.TrafficParams) == 40 == sum(C.sizeof(t) for _, t in engine.TrafficParams._fields_)    # no padding
    assert set(engine.TRAFFIC_DEFAULTS) == {n for _, n in fields} - {"struct_size", "reserved"}
    for fn in ("sg_set_traffic_trend", "sg_window_traffic", "sg_window_node_traffic", "sg_window_group_traffic", "sg_window_group_node_traffic",
               "sg_window_traffic_buffer", "sg_traffic_trend_entries", "sg_traffic_trend_stats_get", "sg_window_nodes_top_traffic",
               "sg_window_groups_top_traffic", "sg_window_group_nodes_top_traffic"):
        assert re.search(r"^int " + fn + r"\(", h, re.M) and fn in engine._SIGNATURES, fn
    assert engine.ABI_VERSION == 6 and "#define SG_ABI_VERSION 6u" in h        # additive: the version does not move
    # the struct's size, every field's offset, size and kind, and the constants, by the compiler: tests/test_abi.py's own check
    from tests import abi_layouts
    src = tmp_path / "traffic_layout_check.c"
    consts = {**{"SG_T_" + k.upper(): v for k, v in engine.T_SPACES.items()}, **{"SG_TSEL_" + k.upper(): v for k, v in engine.TSEL_BY.items()},
              **{"SG_TSEL_" + k.upper(): v for k, v in engine.TSEL_SIDE.items()}}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(abi_layouts, "LAYOUTS", {"sg_traffic_params": engine.TrafficParams})
        mp.setattr(abi_layouts, "CONSTANTS", consts)
        src.write_text(abi_layouts.layout_check_source())
    assert "offsetof(sg_traffic_params, rate_floor) == 32" in src.read_text() and "SG_TSEL_OUT) == 8LL" in src.read_text()
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert EDGE_OUT_DTYPE.fields["count"][0] == np.dtype("<u4") and NODE_DTYPE.fields["in_count"][0] == np.dtype("<u8")   # the two sample types
