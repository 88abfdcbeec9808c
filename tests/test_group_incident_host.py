"""CPU tests of the workload incidents (K18): the reference tests/group_incident_ref.py against a breadth-first search written
apart from it, against K12's reference where the map groups nothing, against K12's incidents under maps that group (every pod
incident lies inside one workload incident), hand cases, and the plan in alaz_amd/csrc/sg_plan.hpp
(tests/micro/plan_driver.cpp, stage group_incident) — layout, sizes at config 3 and at 2^21 keys, the direct path's reach on the small GPU
engine, parameter checks."""
import os
from collections import deque

import numpy as np
import pytest

from alaz_amd import engine, weights
from tests.group_incident_ref import group_incident_ref, red_groups
from tests.group_rank_ref import group_rank_ref
from tests.group_ref import group_of_ref
from tests.helpers import CLOCK, G
from tests.host_scaffold import _okey, contract, incident_rows_of as rows_of
from tests.incident_ref import QUANTILES, incident_ref, quantile_threshold
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.rank_ref import rank_ref
from tests.traces import _random_map, _random_rows
from tests.traces import churn  # noqa: F401  (the fixture: events only, no engine)

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_INCIDENT
NOG = engine.NO_GROUP
INF = float("inf")


def incidents_bfs(ge, gn, values, min_value, rank=None):
    """the contract again, on its own: an adjacency list over the workload rows, a breadth-first search from every unvisited
    endpoint in row order, the summaries by one pass over each component's group edges"""
    n = len(gn)
    at = {int(r): v for v, r in enumerate(gn["ref"])}
    adj = [[] for _ in range(n)]
    mine = [[] for _ in range(n)]                                    # red group edges by source row
    thr = np.float32(min_value)
    for j in range(len(ge)):
        u, v = at.get(int(ge["from_ref"][j])), at.get(int(ge["to_ref"][j]))
        if u is None or v is None or not np.float32(values[j]) >= thr:
            continue
        adj[u].append(v); adj[v].append(u); mine[u].append(j)
    inc = np.full(n, NO, dtype=np.uint32)
    comps = []
    for s in range(n):
        if inc[s] != NO or not adj[s]:
            continue
        inc[s] = len(comps)
        comp, q = [], deque([s])
        while q:
            u = q.popleft()
            comp.append(u)
            for v in adj[u]:
                if inc[v] == NO:
                    inc[v] = len(comps); q.append(v)
        comps.append(sorted(comp))
    out = np.zeros(len(comps), dtype=engine.INCIDENT_DTYPE)
    for i, comp in enumerate(comps):
        js = sorted(j for u in comp for j in mine[u])
        o = out[i]
        o["first_node"], o["nodes"], o["edges"] = comp[0], len(comp), len(js)
        for f, g in (("count", "count"), ("err", "err_count"), ("sum_ns", "sum_ns"), ("score_q32", "score_q32")):
            o[f] = sum(int(ge[g][j]) for j in js) % (1 << 64)
        best = max(_okey(values[j]) for j in js)
        o["worst_row"] = min(j for j in js if _okey(values[j]) == best)
        o["value_max"] = values[o["worst_row"]]
        top = max(_okey(gn["score"][v]) for v in comp)
        o["top_node"] = min(v for v in comp if _okey(gn["score"][v]) == top)
        o["culprit_node"] = NO
        if rank is not None:
            big = max(int(rank["rank"][v]) for v in comp)
            o["culprit_node"] = min(v for v in comp if int(rank["rank"][v]) == big)
            o["rank_sum"] = sum(int(rank["rank"][v]) for v in comp) % (1 << 64)
    return out, inc


VALUES = np.array([0.0, -0.0, 0.25, 0.5, 0.75, 1.0, -1.0, np.nan, -2.5], dtype=np.float32)


def _random_window(rng):
    """group edges over GROUP, KNOWN, LABEL and OBIP refs (self-edges from _random_rows and from pods of one group calling each
    other) and their workload rows; score_max with NaN, -0.0, equal and negative values put in; sums that wrap a u64"""
    mk, ml, mg = int(rng.integers(4, 90)), int(rng.integers(1, 12)), int(rng.integers(1, 20))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 4 * mk)))
    gmap = _random_map(rng, mk, mg, share=float(rng.choice([0.0, 0.5, 1.0])), block=(None, 3)[int(rng.integers(0, 2))])
    ge, gn = contract(rows, gmap, mg, mk, ml)
    put = rng.random(len(ge)) < 0.5
    ge["score_max"][put] = rng.choice(VALUES, int(put.sum()))
    for f in ("count", "err_count", "sum_ns", "score_q32"):
        ge[f] = rng.integers(0, 1 << 63, len(ge), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(ge)).astype(np.uint64)
    kinds = {int(r) >> 30 for r in np.concatenate([ge["from_ref"], ge["to_ref"]])}
    return ge, gn, kinds


@pytest.mark.parametrize("block", range(6))
def test_reference_against_breadth_first_search(block):
    """300 seeds, 50 a case"""
    met, kinds, selfs = set(), set(), 0
    for seed in range(50 * block, 50 * block + 50):
        rng = np.random.default_rng(1800 + seed)
        ge, gn, k = _random_window(rng)
        kinds |= k
        selfs += int((ge["from_ref"] == ge["to_ref"]).sum())
        if seed % 3 == 0 and len(gn) > 4:                             # refs without a workload row: their group edges are never red
            gn = np.delete(gn, rng.choice(len(gn), len(gn) // 5, replace=False))
        trend = np.zeros(len(ge), dtype=engine.TREND_DTYPE)
        trend["lat_dev"] = rng.choice(np.array([0.0, -0.0, 1.5, 3.0, np.nan, -2.0], dtype=np.float32), len(ge))
        trend["err_dev"] = rng.standard_normal(len(ge)).astype(np.float32)
        rank = np.zeros(len(gn), dtype=engine.RANK_DTYPE)
        rank["rank"] = rng.integers(0, 5, len(gn)).astype(np.uint64) << np.uint64(62)   # ties, and a sum that wraps
        by = ("score", "lat_dev", "err_dev")[seed % 3]
        val = ge["score_max"] if by == "score" else trend[by]
        for thr in (-INF, 0.0, quantile_threshold(val, 0.7), INF):
            rk = (None, rank)[seed % 2]
            got, gi = group_incident_ref(ge, gn, by, thr, trend=trend, rank=rk)
            want, wi = incidents_bfs(ge, gn, val, thr, rank=rk)
            assert got.tobytes() == want.tobytes(), (seed, by, thr)
            assert gi.tolist() == wi.tolist()
            met.add(len(got))
            if thr == INF:
                assert len(got) == 0                                  # (no value is +inf)
    assert max(met) > 3 and kinds == {0, 1, 2, 3} and selfs > 0


# ---- under the map that groups nothing the result is K12's -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_windows(churn, oracle_lib):  # noqa: F811
    """the oracle's rows of every churn window"""
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    W = weights.make_weights(2)
    out = []
    for w in wins:
        o.packed(w, labels); o.window_close(W, 2)
        out.append(o.edge_rows())
    return topo, out


def _thresholds(rows):
    return [-INF, INF] + [quantile_threshold(rows["score"], q) for q in QUANTILES]


def test_a_map_that_groups_nothing_gives_k12s_incidents(oracle_windows):
    topo, wins = oracle_windows
    mk = topo.n_nodes + 8
    some = 0
    for rows in wins:
        ge, gn = contract(rows, np.full(mk, NOG, np.uint32), mk, mk, 256)
        nodes = nodes_ref(rows)
        assert len(ge) == len(rows) and gn.tobytes() == nodes.tobytes()
        rk, grk = rank_ref(rows, nodes, iters=3), group_rank_ref(ge, gn, iters=3)
        assert rk.tobytes() == grk.tobytes()
        for thr in _thresholds(rows):
            for a, b in ((None, None), (rk, grk)):
                want, wi = incident_ref(rows, nodes, "score", thr, rank=a)
                got, gi = group_incident_ref(ge, gn, "score", thr, rank=b)
                assert got.tobytes() == want.tobytes() and gi.tobytes() == wi.tobytes()
                some += len(got)
    assert some > 0


@pytest.mark.parametrize("kind", ["blocks", "one"])
def test_every_pod_incident_lies_inside_one_workload_incident(oracle_windows, kind):
    """a red row makes its group edge red (score_max >= score), so a K12 incident's node rows map, by group ref, into exactly one
    K18 incident: the K18 count is at most K12's, and on at least one window it is strictly smaller"""
    topo, wins = oracle_windows
    mk = topo.n_nodes + 8
    gmap = np.full(mk, NOG, np.uint32)
    gmap[:topo.n_pods] = np.arange(topo.n_pods) // 7 if kind == "blocks" else 0
    fewer = False
    for rows in wins[:6]:
        ge, gn = contract(rows, gmap, mk, mk, 256)
        nodes = nodes_ref(rows)
        at = {int(r): v for v, r in enumerate(gn["ref"])}
        wrow = np.array([at[group_of_ref(int(r), gmap)] for r in nodes["ref"]])   # node row -> workload row
        for thr in _thresholds(rows)[2:]:
            pods, pinc = incident_ref(rows, nodes, "score", thr)
            wl, winc = group_incident_ref(ge, gn, "score", thr)
            for i in range(len(pods)):
                inside = set(winc[wrow[pinc == i]].tolist())
                assert len(inside) == 1 and NO not in inside, (thr, i, inside)
            assert len(wl) <= len(pods)
            fewer |= len(wl) < len(pods)
    assert fewer


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------
def test_no_red_group_edge_gives_no_incident():
    ge, gn = contract(rows_of((1, 2, 0.1), (2, 3, 0.2)), [NOG] * 8, 4, 8, 1)
    out, inc = group_incident_ref(ge, gn, "score", 0.5)
    assert len(out) == 0 and inc.tolist() == [NO] * 3
    nan, nn = contract(rows_of((1, 2, float("nan"))), [NOG] * 8, 4, 8, 1)
    assert len(group_incident_ref(nan, nn, "score", -INF)[0]) == 0    # NaN is never red, not even at -inf
    assert len(group_incident_ref(ge[:0], gn[:0], "score", -INF)[0]) == 0


def test_a_red_group_edge_inside_a_workload_alone_is_an_incident():
    # pods 1 and 2 of group 0 call each other (red); 5 -> 6 is quiet
    ge, gn = contract(rows_of((1, 2, 0.9), (2, 1, 0.7), (5, 6, 0.1)), [NOG, 0, 0, NOG, NOG, NOG, NOG, NOG], 4, 8, 1)
    assert gn["ref"].tolist() == [G(0), 5, 6] and ge["from_ref"].tolist() == [G(0), 5] and ge["edges"].tolist() == [2, 1]
    out, inc = group_incident_ref(ge, gn, "score", 0.5)
    assert inc.tolist() == [0, NO, NO]
    o = out[0]
    assert (o["nodes"], o["edges"], o["first_node"], o["top_node"], o["worst_row"]) == (1, 1, 0, 0, 0)
    assert o["count"] == 10 + 11 and o["value_max"] == np.float32(0.9)    # both rows of the group edge count; its value is score_max


def test_two_chains_are_numbered_by_their_smallest_row_and_sums_are_the_group_edges_fields():
    # groups: 0 = {1, 2}, 1 = {3}; ungrouped 5 .. 9.  Chains g0 -> 5 -> 9 (pods 1 and 2 both call 5) and 7 -> g1 -> 8
    gmap = [NOG, 0, 0, 1] + [NOG] * 8
    rows = rows_of((1, 5, 0.9), (2, 5, 0.1), (5, 9, 0.8), (7, 3, 0.7), (3, 8, 0.95))
    ge, gn = contract(rows, gmap, 4, 12, 1)
    assert gn["ref"].tolist() == [G(0), G(1), 5, 7, 8, 9]
    assert list(zip(ge["from_ref"].tolist(), ge["to_ref"].tolist())) == [(G(0), 5), (G(1), 8), (5, 9), (7, G(1))]
    out, inc = group_incident_ref(ge, gn, "score", 0.5)
    assert inc.tolist() == [0, 1, 0, 1, 1, 0]
    assert out["first_node"].tolist() == [0, 1] and out["nodes"].tolist() == [3, 3] and out["edges"].tolist() == [2, 2]
    # rows sorted: (1,5) (2,5) (3,8) (5,9) (7,3) with count 10 .. 14: the quiet row (2,5) counts, it is folded into a red group edge
    assert out["count"].tolist() == [10 + 11 + 13, 12 + 14] and out["err"].tolist() == [0 + 1 + 3, 2 + 4]
    assert out["score_q32"].tolist() == [int(ge["score_q32"][0]) + int(ge["score_q32"][2]), int(ge["score_q32"][1]) + int(ge["score_q32"][3])]
    assert out["worst_row"].tolist() == [0, 1] and out["value_max"].tolist() == [np.float32(0.9), np.float32(0.95)]
    assert out["culprit_node"].tolist() == [NO, NO] and out["rank_sum"].tolist() == [0, 0] and out["reserved"].tolist() == [0, 0]


def test_a_bridge_that_is_not_red_joins_nothing():
    ge, gn = contract(rows_of((1, 2, 0.9), (2, 3, 0.1), (3, 4, 0.9)), [NOG] * 8, 4, 8, 1)
    out, inc = group_incident_ref(ge, gn, "score", 0.5)
    assert inc.tolist() == [0, 0, 1, 1] and out["edges"].tolist() == [1, 1]
    one, inc1 = group_incident_ref(ge, gn, "score", 0.1)
    assert inc1.tolist() == [0] * 4 and one["edges"].tolist() == [3] and one["nodes"].tolist() == [4]


def test_a_ref_without_a_row_is_never_red():
    ge, gn = contract(rows_of((1, 2, 0.9), (2, 3, 0.9)), [NOG] * 8, 4, 8, 1)
    out, inc = group_incident_ref(ge, gn[:2], "score", -INF)           # ref 3's row cut
    assert inc.tolist() == [0, 0] and out["edges"].tolist() == [1]
    val, red, src, dst = red_groups(ge, gn[:2], "score", -INF)
    assert red.tolist() == [True, False] and dst.tolist() == [1, -1]


def test_ties_go_to_the_smallest_index_and_worst_row_is_a_group_edge_index():
    # group 0 = pods 1, 2, 3, 4: six rows fold into group edges g0 -> 6, g0 -> 7, 6 -> 8; the worst POD row is row 3, the worst
    # GROUP EDGE is 1 — worst_row names the group edge, whose own worst_row (3) leads to the pod row
    gmap = [NOG, 0, 0, 0, 0] + [NOG] * 7
    rows = rows_of((1, 6, 0.2), (2, 6, 0.5), (3, 7, 0.1), (4, 7, 0.5), (6, 8, 0.5))
    ge, gn = contract(rows, gmap, 4, 12, 1)
    assert ge["score_max"].tolist() == [0.5, 0.5, 0.5] and ge["worst_row"].tolist() == [1, 3, 4]
    rank = group_rank_ref(ge, gn)
    rank["rank"] = [7, 9, 9, 3]
    out, _ = group_incident_ref(ge, gn, "score", -INF, rank=rank)
    assert len(out) == 1 and out["worst_row"][0] == 0 and out["value_max"][0] == np.float32(0.5)
    assert gn["score"].tolist() == [0.5] * 4 and out["top_node"][0] == 0
    assert out["culprit_node"][0] == 1 and out["rank_sum"][0] == 28
    out2, _ = group_incident_ref(ge, gn, "score", -INF)
    ge2 = ge.copy(); ge2["score_max"][0] = 0.25
    assert group_incident_ref(ge2, gn, "score", -INF)[0]["worst_row"][0] == 1 and int(ge["worst_row"][1]) == 3
    zero, zn = contract(rows_of((1, 2, -0.0), (2, 3, 0.0), (3, 4, 0.0)), [NOG] * 8, 4, 8, 1)
    z, _ = group_incident_ref(zero, zn, "score", 0.0)                 # -0.0 >= 0.0: red; +0.0 is above it, its first group edge wins
    assert z["edges"][0] == 3 and z["worst_row"][0] == 1 and not np.signbit(z["value_max"][0])


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("group_incident")


def _p(me, ncap, mg, slots=1, rows=0, ge=0, ss=16, by=0, res=0):
    return (me, ncap, mg, slots, rows, ge, ss, by, res)


# toy, config 2, config 3 (15 k node ids, as many groups), a config-5 shard, K16's 2^21-key limit, degenerate
ENGINES = [(4096, 1100, 1000), (1 << 15, 1076, 1076), (1_250_000, 15_000, 15_000), (2_750_000, 400_000, 100_000),
           (4_000_000, 1 << 20, 1 << 20), (1, 1, 1), (0, 0, 0)]


def test_plan_sizes_and_layout(plan):
    for r in plan([_p(me, nc, mg, slots) for me, nc, mg in ENGINES for slots in (1, 3, 8)]):
        assert r["rc"] == 0 and r["out_size"] == 72 and r["params_size"] == 16
        me, slots = max(r["max_edges"], 1), r["slots"]
        gk, nc = max(r["gk"], 1), max(r["nc"], 1)
        assert r["gk"] == r["ncap"] + r["max_groups"] and r["nc"] == min(gk, 2 * me)
        assert r["threads"] == 256 and r["node_per"] % 256 == 0 and 1 <= r["node_wgs"] <= r["max_wgs"] == 1024
        assert r["node_wgs"] * r["node_per"] >= nc > (r["node_wgs"] - 1) * r["node_per"]
        assert 1 <= r["grid_wgs"] <= 1024 and 1 <= r["hook_wgs"] <= 1024 and 1 <= r["row_wgs"] <= r["max_row_wgs"] == 256
        assert r["row_wgs"] == min(r["hook_wgs"], 256)
        assert r["fold_rounds"] == 8 and r["fold_wgs"] == max(1, min(1024, -(-nc // 2048)))
        need = {"pos": 4 * gk, **{k: 4 * nc for k in ("parent", "flag", "lab", "num", "stage", "stage_idx", "node_inc")}, "esrc": 4 * me,
                "keys": 24 * nc, "blk": 2 * 1024 * 4, "rows": 72 * nc, "count": 8}
        check_layout(r, need, per_slot=("rows", "count", "node_inc"))
        # 4 B a key, 4 B a group edge, 48 + 76 x slots B a row, the head counts, 256 B of rounding a piece: nothing else
        assert r["total_bytes"] <= 4 * gk + 4 * me + (48 + 76 * slots) * nc + 8192 + 256 * (10 + 4 * slots)


def test_plan_at_config_3_and_at_the_key_limit(plan):
    c3, = plan([_p(1_250_000, 15_000, 15_000, slots=2, rows=5_600, ge=590_000)])
    assert (c3["gk"], c3["nc"]) == (30_000, 30_000)
    assert (c3["node_wgs"], c3["node_per"], c3["grid_wgs"], c3["fold_wgs"], c3["hook_wgs"], c3["row_wgs"]) == (118, 256, 118, 15, 1024, 256)
    assert c3["total_bytes"] == 11_129_856                             # 10.6 MiB: 4.8 of it esrc, 4.4 the two slots' rows
    lim, = plan([_p(4_000_000, 1 << 20, 1 << 20, slots=2)])
    assert (lim["gk"], lim["nc"], lim["node_wgs"], lim["node_per"], lim["fold_wgs"]) == (1 << 21, 1 << 21, 1024, 2048, 1024)
    assert lim["total_bytes"] < 440 << 20


def test_the_small_gpu_engine_reaches_the_direct_path(plan):
    """tests/test_gpu_group_incidents.py: max_edges 4096 over more than 8192 pods, 4096 disjoint red pairs 2i -> 2i + 1 — one
    workgroup of each folding pass meets more distinct incidents than its LDS table has slots"""
    r, = plan([_p(4096, 8192 + 8 + 16 + 64, 8192 + 8, rows=8192, ge=4096)])
    assert r["nc"] == 8192 and (r["fold_wgs"], r["row_wgs"]) == (4, 4)
    assert r["fold_rows"] // 2 == 1024 > r["table_slots"] == 512       # k18_nodes: 2048 rows, two a pair
    assert r["row_edges"] == 1024 > r["table_slots"]                   # k18_rows: 1024 group edges, each its own incident


def test_plan_parameter_checks(plan):
    ok = plan([_p(1000, 100, 10, by=b) for b in (0, 1, 2)])
    assert [r["rc"] for r in ok] == [0] * 3 and [r["by"] for r in ok] == [0, 1, 2]
    bad = plan([_p(1000, 100, 10, by=3), _p(1000, 100, 10, by=4), _p(1000, 100, 10, ss=12), _p(1000, 100, 10, ss=20), _p(1000, 100, 10, res=1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
