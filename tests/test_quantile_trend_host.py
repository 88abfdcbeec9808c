"""CPU tests of the tail baselines (K21): the numpy references of tests/quantile_trend_ref.py against a second formulation written
apart from them (a dict keyed by (from_key, to_key), plain Python floats, one sample at a time), against hand-computed answers and
against the mean baselines' references (the error half is theirs), the scenario the stage is for — a tail regression the mean
baseline does not see — and the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage quantile_trend)."""
import os

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.engine import GROUP_EDGE_DTYPE, NODE_DTYPE, NO_GROUP as NO
from tests.group_nodes_ref import GroupNodeTrendRef, group_nodes_ref
from tests.group_ref import group_ref
from tests.group_trend_ref import GroupTrendRef, group_keys, workload_keys
from tests.node_trend_ref import NodeTrendRef
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout, check_soa
from tests import quantile_ref as qr
from tests.quantile_trend_ref import GroupTailRef, NodeTailRef, WorkloadTailRef
from tests.traces import _random_map, _random_rows
from tests.trend_ref import ref_keys

HERE = os.path.dirname(os.path.abspath(__file__))
U32_MAX = 0xFFFFFFFF
PERMILLE = (500, 990, 999)


# ---- the second formulation -------------------------------------------------------------------------------------------------------
class DictTail:
    """one baseline as a dict: key -> [lat_mean, lat_dev, err_mean, err_dev, n, last].  window(samples) takes the window's samples
    (key, count, err, Q) in key order and returns their (lat_dev, err_dev, base_mean_us, seen)"""

    def __init__(self, cap, shift, warmup, ttl, lat_floor=1000.0, err_floor=10486.0):
        self.cap, self.alpha, self.warmup, self.ttl, self.lat_floor, self.err_floor = cap, 2.0 ** -shift, warmup, ttl, lat_floor, err_floor
        self.d, self.w = {}, 0
        self.stats = dict(windows=0, entries=0, inserted=0, expired=0, dropped=0)

    def window(self, samples):
        self.w += 1
        out, updates, fresh = [], [], []
        for key, c, err, q in samples:
            e = self.d.get(key)
            xl, xe = 1000.0 * float(q), float((int(err) << 20) // int(c)) if c else 0.0
            ld = ed = base = np.float32(0.0)
            seen = 0
            if e is not None:
                seen, base = e[4], np.float32(e[0] / 1000.0)
                if c > 0 and seen >= self.warmup:
                    ld = np.float32((xl - e[0]) / (e[1] if e[1] > self.lat_floor else self.lat_floor))
                    ed = np.float32((xe - e[2]) / (e[3] if e[3] > self.err_floor else self.err_floor))
            out.append((ld, ed, base, seen))
            if c > 0:
                (updates if e is not None else fresh).append((key, xl, xe))
        touched = set()
        for key, xl, xe in updates:                                   # after every row was scored: from the entries as they stood
            e = self.d[key]
            dl, de = xl - e[0], xe - e[2]
            e[0] = e[0] + dl * self.alpha; e[1] = e[1] + (abs(dl) - e[1]) * self.alpha
            e[2] = e[2] + de * self.alpha; e[3] = e[3] + (abs(de) - e[3]) * self.alpha
            e[4] = min(e[4] + 1, U32_MAX); e[5] = self.w
            touched.add(key)
        for key in [k for k, e in self.d.items() if k not in touched and self.w - e[5] >= self.ttl]:
            del self.d[key]; self.stats["expired"] += 1
        room = max(self.cap - len(self.d), 0)
        for key, xl, xe in sorted(fresh)[:room]:
            self.d[key] = [xl, 0.0, xe, 0.0, 1, self.w]
        s = self.stats
        s["windows"] += 1; s["entries"] = len(self.d); s["inserted"] += min(len(fresh), room); s["dropped"] += len(fresh) - min(len(fresh), room)
        return out

    def entries(self):
        return [(k[0], k[1], *self.d[k]) for k in sorted(self.d)]


def _entries_of(ref):
    e = ref.entries
    return [(int(a), int(b), float(c), float(d), float(f), float(g), int(h), int(i)) for a, b, c, d, f, g, h, i in
            zip(e["from_key"], e["to_key"], e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"])]


def _node_samples(nodes, q, keys):
    """node (or workload) rows one side at a time: the IN side of row k — side 0 — takes the table's entry [k][1], the OUT side [k][0]"""
    out = []
    for k in range(len(nodes)):
        out.append(((int(keys[k]), 0), int(nodes["in_count"][k]), int(nodes["in_err"][k]), int(q[k][1])))
        out.append(((int(keys[k]), 1), int(nodes["out_count"][k]), int(nodes["out_err"][k]), int(q[k][0])))
    return out


def _node_rows(out):
    got = np.zeros(len(out) // 2, dtype=engine.NODE_TREND_DTYPE)
    for j, (ld, ed, base, seen) in enumerate(out):
        s = "in" if j % 2 == 0 else "out"
        got[f"{s}_lat_dev"][j // 2], got[f"{s}_err_dev"][j // 2], got[f"{s}_base_mean_us"][j // 2], got[f"{s}_seen"][j // 2] = ld, ed, base, seen
    return got


def _hist(rng, rows):
    """a histogram per row: a few bins set, none for a row without requests"""
    h = np.zeros((len(rows), 16), dtype=np.uint32)
    for i in range(len(rows)):
        if rows["count"][i]:
            for b in rng.integers(0, 16, int(rng.integers(1, 4))):
                h[i, b] += rng.integers(1, 1000)
    return h


@pytest.mark.parametrize("block", range(8))
def test_references_against_the_dict_formulation(block):
    """40 seeds a block: chains of 6 - 10 windows of random rows under maps that group nothing, something and everything; every
    window's tail rows, and the baseline and the statistics after it, in all three spaces"""
    for seed in range(40 * block, 40 * block + 40):
        rng = np.random.default_rng(9000 + seed)
        mk, ml = int(rng.integers(41, 80)), int(rng.integers(1, 8))      # (_random_rows makes pods of ids below 40 whatever mk is)
        mg = int(rng.integers(1, mk + 1))
        gmap = (np.full(mk, NO, np.uint32), _random_map(rng, mk, mg), np.zeros(mk, np.uint32))[seed % 3]
        p = dict(shift=int(rng.integers(1, 5)), warmup=int(rng.integers(1, 4)), ttl=int(rng.integers(1, 5)), max_entries=int(rng.integers(3, 80)))
        qi = int(rng.integers(0, len(PERMILLE)))
        ncap, nc = mk + ml + 40, mg + mk + ml + 40
        refs = NodeTailRef(ncap, **p), GroupTailRef(1 << 12, **p), WorkloadTailRef(nc, **p)
        dicts = [DictTail(p["max_entries"], p["shift"], p["warmup"], p["ttl"]) for _ in range(3)]
        for w in range(int(rng.integers(6, 11))):
            rows = _random_rows(rng, mk, ml, int(rng.integers(0, 120)))
            obips = np.sort(rng.choice(1 << 24, 40, replace=False)).astype(np.uint32) + np.uint32(1 << 24)
            hist = _hist(rng, rows)
            nodes = nodes_ref(rows)
            ge, _, perm = group_ref(rows, gmap, mg, mk, ml)
            gn = group_nodes_ref(ge, mg, mk, ml)
            qn = qr.node_quantiles(qr.fold_nodes(hist, rows, nodes), nodes, PERMILLE)[:, :, qi]
            qg = qr.group_quantiles(qr.fold_groups(hist, ge, perm), ge, PERMILLE)[:, qi]
            qw = qr.node_quantiles(qr.fold_group_nodes(hist, ge, perm, gn), gn, PERMILLE)[:, :, qi]
            # nodes
            want = refs[0].window(nodes, qn, obips)
            got = _node_rows(dicts[0].window(_node_samples(nodes, qn, ref_keys(nodes["ref"], obips))))
            assert got.tobytes() == want.tobytes(), (seed, w)
            # group edges
            want = refs[1].window(ge, qg, obips)
            fk, tk = group_keys(ge, obips)
            out = dicts[1].window([((int(fk[j]), int(tk[j])), int(ge["count"][j]), int(ge["err_count"][j]), int(qg[j])) for j in range(len(ge))])
            got = np.zeros(len(ge), dtype=engine.TREND_DTYPE)
            for j, (ld, ed, base, seen) in enumerate(out):
                got["lat_dev"][j], got["err_dev"][j], got["base_mean_us"][j], got["windows_seen"][j] = ld, ed, base, seen
            assert got.tobytes() == want.tobytes(), (seed, w)
            # workloads
            want = refs[2].window(gn, qw, obips)
            got = _node_rows(dicts[2].window(_node_samples(gn, qw, workload_keys(gn["ref"], obips))))
            assert got.tobytes() == want.tobytes(), (seed, w)
            for r, d in zip(refs, dicts):
                assert _entries_of(r) == d.entries() and r.stats == d.stats, (seed, w)


# ---- hand-computed answers ----------------------------------------------------------------------------------------------------------
def _ge(pairs):
    """group edges (from group, to group, count, err_count), ascending"""
    g = np.zeros(len(pairs), dtype=GROUP_EDGE_DTYPE)
    for i, (f, t, c, e) in enumerate(pairs):
        g["from_ref"][i], g["to_ref"][i], g["count"][i], g["err_count"][i] = (engine.REF_GROUP << 30) | f, (engine.REF_GROUP << 30) | t, c, e
    return g


def _entry(ref, f, t):
    e = ref.entries
    return e[(e["from_key"] == f) & (e["to_key"] == t)]


def test_one_entity_by_hand_warmup_an_octave_jump_expiry_and_the_capacity_cut():
    """workload edge 3 -> 5 with alpha = 1/2, warmup 2, ttl 2, two entries at most"""
    ref = GroupTailRef(100, shift=1, warmup=2, ttl=2, max_entries=2)
    ob = np.zeros(0, np.uint32)
    X = _ge([(3, 5, 3, 1)])
    t = ref.window(X, [1000], ob)[0]                                  # w1: a new entry; the row is zero
    assert (t["lat_dev"], t["err_dev"], t["base_mean_us"], t["windows_seen"]) == (0, 0, 0, 0)
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["err_mean"], e["err_dev"], e["n"], e["last"]) == (1_000_000.0, 0.0, 349525.0, 0.0, 1, 1)   # floor(2^20 / 3)
    t = ref.window(X, [1000], ob)[0]                                  # w2: seen 1 < warmup: the base only
    assert (t["lat_dev"], t["err_dev"], t["base_mean_us"], t["windows_seen"]) == (0, 0, 1000.0, 1)
    t = ref.window(X, [2000], ob)[0]                                  # w3: the quantile one octave up; dev 0: the floor of 1000 ns
    assert (t["lat_dev"], t["base_mean_us"], t["windows_seen"]) == (1000.0, 1000.0, 2)
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["n"], e["last"]) == (1_500_000.0, 500_000.0, 3, 3)
    t = ref.window(X, [2000], ob)[0]                                  # w4: (2e6 - 1.5e6) / 5e5
    assert (t["lat_dev"], t["base_mean_us"], t["windows_seen"]) == (1.0, 1500.0, 3)
    e = _entry(ref, 3, 5)[0]
    assert (e["lat_mean"], e["lat_dev"], e["n"], e["last"]) == (1_750_000.0, 500_000.0, 4, 4)
    O = _ge([(4, 4, 1, 0)])
    ref.window(O, [7], ob)                                            # w5: X silent for one window: kept
    assert len(_entry(ref, 3, 5)) == 1 and ref.stats["entries"] == 2
    alive = ref.window(_ge([(3, 5, 0, 0), (4, 4, 1, 0)]), [0, 7], ob)[0]    # w6: an alive-only sample does not refresh: 6 - 4 = ttl, expired
    assert (alive["lat_dev"], alive["base_mean_us"], alive["windows_seen"]) == (0, 1750.0, 4)
    assert len(_entry(ref, 3, 5)) == 0 and ref.stats["expired"] == 1 and ref.stats["entries"] == 1
    # w7: three new keys beside the kept one: room for the first in key order only
    ref.window(_ge([(3, 5, 2, 0), (4, 4, 1, 0), (6, 1, 1, 0), (9, 9, 1, 0)]), [4000, 7, 1, 1], ob)
    assert [(int(a), int(b)) for a, b in zip(ref.entries["from_key"], ref.entries["to_key"])] == [(3, 5), (4, 4)]
    assert ref.stats == dict(windows=7, entries=2, inserted=3, expired=1, dropped=2)
    assert _entry(ref, 3, 5)[0]["lat_mean"] == 4_000_000.0 and _entry(ref, 3, 5)[0]["n"] == 1


def _node_row(ref, in_c=0, in_sum=0, in_max=0, out_c=0, out_sum=0, out_max=0):
    n = np.zeros(1, dtype=NODE_DTYPE)
    n["ref"], n["in_count"], n["in_sum_ns"], n["in_max_ns"] = ref, in_c, in_sum, in_max
    n["out_count"], n["out_sum_ns"], n["out_max_ns"] = out_c, out_sum, out_max
    return n


def test_the_side_mapping():
    """a node called slowly and calling quickly: the table's side [0] is OUT, the sample's side 0 is IN"""
    nodes = _node_row(7, in_c=10, in_sum=80_000_000, in_max=9_000_000, out_c=10, out_sum=10_000_000, out_max=1_100_000)
    hist = np.zeros((1, 2, 16), np.uint64)
    hist[0, 0, 4] = 10                                                # out: 1 ms, bin 4 [2^20, 2^21)
    hist[0, 1, 7] = 10                                                # in: 8 ms, bin 7 [2^23, 2^24)
    q = qr.node_quantiles(hist, nodes, (990,))[:, :, 0]
    assert q.tolist() == [[1100, 9000]]                               # each below its bin's upper edge: capped by the side's own max
    ob = np.zeros(0, np.uint32)
    for Ref, key in ((NodeTailRef, 7), (WorkloadTailRef, (1 << 32) + 7)):
        ref = Ref(16, shift=1, warmup=1)
        ref.window(nodes, q, ob)
        e = ref.entries
        assert e["from_key"].tolist() == [key, key] and e["to_key"].tolist() == [0, 1]
        assert e["lat_mean"].tolist() == [9_000_000.0, 1_100_000.0]   # (key, 0) = in, (key, 1) = out
        t = ref.window(nodes, q[:, ::-1], ob)[0]                      # the sides swapped: each deviates the other way
        assert t["in_base_mean_us"] == 9000.0 and t["out_base_mean_us"] == 1100.0
        assert t["in_lat_dev"] == np.float32((1_100_000.0 - 9_000_000.0) / 1000.0) and t["out_lat_dev"] == np.float32((9_000_000.0 - 1_100_000.0) / 1000.0)


# ---- identities with the mean baselines ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_the_error_half_is_the_mean_baselines_and_an_empty_map_gives_the_node_space(seed):
    rng = np.random.default_rng(700 + seed)
    mk, ml = 50, 5
    p = dict(shift=2, warmup=2, ttl=3, max_entries=60)
    nothing = np.full(mk, NO, np.uint32)
    gmap = nothing if seed % 2 == 0 else _random_map(rng, mk, 6)
    ncap = mk + ml + 40
    tails = NodeTailRef(ncap, **p), GroupTailRef(1 << 12, **p), WorkloadTailRef(ncap, **p)
    means = NodeTrendRef(ncap, **p), GroupTrendRef(1 << 12, **p), GroupNodeTrendRef(ncap, **p)
    for w in range(8):
        rows = _random_rows(rng, mk, ml, 60)
        obips = np.sort(rng.choice(1 << 24, 40, replace=False)).astype(np.uint32) + np.uint32(1 << 24)
        hist = _hist(rng, rows)
        nodes = nodes_ref(rows)
        ge, _, perm = group_ref(rows, gmap, mk, mk, ml)
        gn = group_nodes_ref(ge, mk, mk, ml)
        qn = qr.node_quantiles(qr.fold_nodes(hist, rows, nodes), nodes, (990,))[:, :, 0]
        qg = qr.group_quantiles(qr.fold_groups(hist, ge, perm), ge, (990,))[:, 0]
        qw = qr.node_quantiles(qr.fold_group_nodes(hist, ge, perm, gn), gn, (990,))[:, :, 0]
        t = tails[0].window(nodes, qn, obips), tails[1].window(ge, qg, obips), tails[2].window(gn, qw, obips)
        m = means[0].window(nodes, obips), means[1].window(ge, obips), means[2].window(gn, obips)
        for k, fields in ((0, ("in_err_dev", "out_err_dev", "in_seen", "out_seen")), (1, ("err_dev", "windows_seen")),
                          (2, ("in_err_dev", "out_err_dev", "in_seen", "out_seen"))):
            for f in fields:
                assert t[k][f].tobytes() == m[k][f].tobytes(), (k, f)
            for f in ("from_key", "to_key", "err_mean", "err_dev", "n", "last"):
                assert tails[k].entries[f].tobytes() == means[k].entries[f].tobytes(), (k, f)
            assert tails[k].stats == means[k].stats
        if gmap is nothing:
            assert t[2].tobytes() == t[0].tobytes()
            a, b = tails[2].entries, tails[0].entries
            assert np.array_equal(a["from_key"], b["from_key"] + np.uint64(1 << 32))
            for f in ("to_key", "lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last"):
                assert a[f].tobytes() == b[f].tobytes(), f


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------
def _bins(d):
    """the row histogram's rule: bin 0 below 2^17 ns, then an octave a bin, bin 15 from 2^31"""
    b = np.zeros(16, np.uint64)
    for x in d:
        b[0 if x < (1 << 17) else min(int(x).bit_length() - 17, 15)] += 1
    return b


def test_a_tail_regression_the_mean_baseline_does_not_see():
    """1000 requests a window to one callee: a share that varies from window to window takes 0.55 ms, the rest 1.0 ms — the mean
    wobbles by more than a tenth, the p99 stands still.  Then fifteen requests in a thousand take 16 ms, four octaves up.  The
    mean moves by about a quarter, a few times its wobble; the p99 moves by 15 ms against a baseline that never moved.  m, the
    threshold, is the geometric mean of the two deviations the references report: the tail crosses it, the mean stays far below"""
    rng = np.random.default_rng(5)
    p = dict(shift=3, warmup=4)
    tail, mean = NodeTailRef(8, **p), NodeTrendRef(8, **p)
    ob = np.zeros(0, np.uint32)
    calm = []
    for w in range(30):
        fast = int(rng.integers(300, 700))
        d = np.concatenate([np.full(fast, 550_000), np.full(1000 - fast, 1_000_000)]).astype(np.uint64)
        if w == 29:
            d[:15] = 16_000_000
        nodes = _node_row(5, in_c=len(d), in_sum=int(d.sum()), in_max=int(d.max()))
        hist = np.zeros((1, 2, 16), np.uint64); hist[0, 1] = _bins(d)
        q = qr.node_quantiles(hist, nodes, (500, 990))[:, :, 1]
        t, m = tail.window(nodes, q, ob)[0], mean.window(nodes, ob)[0]
        if 4 < w < 29:
            assert t["in_lat_dev"] == 0                               # the p99 stands still
            calm.append(abs(float(m["in_lat_dev"])))
    td, md = float(t["in_lat_dev"]), float(m["in_lat_dev"])
    thr = (td * md) ** 0.5
    assert md > 0 and td > thr > md and td > 100 * md
    assert md < 4 * max(calm)                                         # the mean's deviation is of the order of its calm-window wobble
    assert t["in_base_mean_us"] == 1000.0 and q.tolist() == [[0, 16000]]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("quantile_trend")


def _p(spaces=7, on=7, permille=990, qm=(500, 990), ncap=1000, me=4096, nc=1500, slots=1, ss=40, shift=0, warmup=0, ttl=0, maxe=0, lf=0, ef=0, res=0):
    return (spaces, on, permille, len(qm), *(tuple(qm) + (0,) * 8)[:8], ncap, me, nc, slots, ss, shift, warmup, ttl, maxe, lf, ef, res)


def test_plan_is_the_mean_baselines_plan_per_space_in_64_bits(plan):
    cases = [_p(ncap=n, me=me, nc=nc, slots=s) for n, me, nc in ((1, 1, 1), (300, 1 << 15, 700), (70_000, 1_250_000, 140_000), (1 << 21, 1 << 31, 1 << 21))
             for s in (1, 3)] + [_p(maxe=m) for m in (1, 7, 1 << 20)]
    for r in plan(cases):
        assert r["rc"] == 0 and r["spaces"] == 7 and r["qi"] == 1 and r["node_trend_size"] == 32 and r["trend_size"] == 16
        n, me, nc = r["ncap"], r["max_edges"], r["nc"]
        for k, (samples, rows, row) in enumerate(((2 * n, n, 32), (me, me, 16), (2 * nc, nc, 32))):
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
    big, = plan([_p(ncap=1 << 21, me=1 << 31, nc=1 << 21)])
    g = big["sp"][1]
    assert g["entries"] == 1 << 31 and g["rows_bytes"] == 16 << 31 and g["soa_bytes"] >= 56 << 31 and g["total_bytes"] > 1 << 37    # past 2^32
    assert big["sp"][0]["entries"] == 4 << 21 and big["sp"][2]["entries"] == 4 << 21


def test_plan_capacity_defaults_the_tracked_index_and_what_is_refused(plan):
    d, = plan([_p(ncap=1000, me=4096, nc=1500)])
    assert [t["max_entries"] for t in d["sp"]] == [4000, 8192, 6000]  # plan_node_trend's rule, plan_group_trend's, the workloads'
    assert all((t["shift"], t["warmup"], t["ttl"], t["lat_floor_ns"], t["err_floor"]) == (4, 4, 64, 1000, 10486) for t in d["sp"])
    one, = plan([_p(spaces=2, on=6)])
    assert one["spaces"] == 2 and one["sp"][0] is None and one["sp"][2] is None and one["total_bytes"] == one["sp"][1]["total_bytes"]
    eight = (1, 250, 500, 750, 900, 990, 999, 1000)
    assert [r["qi"] for r in plan([_p(permille=q, qm=eight) for q in (1, 750, 1000)])] == [0, 3, 7]
    assert plan([_p(permille=500, qm=(500, 990, 500))])[0]["qi"] == 0  # twice in the set: the first position
    bad = plan([_p(spaces=0), _p(spaces=8), _p(spaces=15), _p(permille=991), _p(permille=990, qm=()), _p(permille=0, qm=(500,)),
                _p(shift=11), _p(ss=36), _p(res=1), _p(maxe=(1 << 31) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * len(bad)
    off = plan([_p(spaces=1, on=6), _p(spaces=7, on=3), _p(spaces=4, on=0)])
    assert [r["rc"] for r in off] == [engine.SG_ESTATE] * 3
    assert plan([_p(spaces=9, on=0)])[0]["rc"] == engine.SG_EINVAL    # unknown bits before the state
