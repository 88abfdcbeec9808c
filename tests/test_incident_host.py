"""CPU tests of the incidents (K12): the reference tests/incident_ref.py against an independent breadth-first implementation on
random row sets, hand cases that pin the contract, the reference's invariants over the oracle's rows of the churn windows (and what
the GPU tests' quantile thresholds cover there), and the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage incident)."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

from alaz_amd import engine, weights
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.helpers import CLOCK
from tests.host_scaffold import _okey, incident_rows_of as rows_of
from tests.incident_ref import QUANTILES, incident_ref, quantile_threshold, red_rows
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.rank_ref import rank_ref
from tests.traces import churn  # noqa: F401  (the fixture: events only, no engine)

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_INCIDENT
INF = float("inf")


def incidents_bfs(rows, nodes, values, min_value, rank=None):
    """the contract again, on its own: an adjacency list over the node rows, a breadth-first search from every unvisited endpoint
    in node order, the summaries by one pass over each component's rows"""
    n = len(nodes)
    at = {int(r): v for v, r in enumerate(nodes["ref"])}
    adj = [[] for _ in range(n)]
    mine = [[] for _ in range(n)]                                    # red rows by source node
    thr = np.float32(min_value)
    for j in range(len(rows)):
        u, v = at.get(int(rows["from_ref"][j])), at.get(int(rows["to_ref"][j]))
        x = np.float32(values[j])
        if u is None or v is None or not x >= thr:
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
        o["count"] = sum(int(rows["count"][j]) for j in js) % (1 << 64)
        o["err"] = sum(int(rows["err_count"][j]) for j in js) % (1 << 64)
        o["sum_ns"] = sum(int(rows["sum_ns"][j]) for j in js) % (1 << 64)
        o["score_q32"] = sum(int(np.float64(rows["score"][j]) * 2.0 ** 32) for j in js if rows["score"][j] > 0) % (1 << 64)
        best = max(_okey(values[j]) for j in js)
        o["worst_row"] = min(j for j in js if _okey(values[j]) == best)
        o["value_max"] = values[o["worst_row"]]
        top = max(_okey(nodes["score"][v]) for v in comp)
        o["top_node"] = min(v for v in comp if _okey(nodes["score"][v]) == top)
        o["culprit_node"] = NO
        if rank is not None:
            big = max(int(rank["rank"][v]) for v in comp)
            o["culprit_node"] = min(v for v in comp if int(rank["rank"][v]) == big)
            o["rank_sum"] = sum(int(rank["rank"][v]) for v in comp) % (1 << 64)
    return out, inc


def _random_rows(rng, n_nodes, n_rows):
    """rows over Known, Label and outbound-IP refs with self-loops, NaN, -0.0, equal and negative scores; huge counts (wrapping sums)"""
    kinds = rng.integers(0, 3, n_nodes).astype(np.uint32)
    refs = np.unique((kinds << np.uint32(30)) | rng.integers(0, 4 * n_nodes, n_nodes).astype(np.uint32))
    f = refs[rng.integers(0, len(refs), n_rows)]
    t = np.where(rng.random(n_rows) < 0.08, f, refs[rng.integers(0, len(refs), n_rows)])
    pairs = np.unique(np.stack([f, t], 1), axis=0)                   # canonical order: ascending (from, to), no duplicates
    r = np.zeros(len(pairs), dtype=EDGE_OUT_DTYPE)
    r["from_ref"], r["to_ref"] = pairs[:, 0], pairs[:, 1]
    s = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.75, 1.0, -1.0, np.nan], dtype=np.float32), len(r))
    s = np.where(rng.random(len(r)) < 0.5, rng.random(len(r)).astype(np.float32), s).astype(np.float32)
    r["score"] = s
    r["count"] = rng.integers(0, 1 << 32, len(r)); r["err_count"] = rng.integers(0, 1 << 20, len(r))
    r["sum_ns"] = rng.integers(0, 1 << 63, len(r), dtype=np.uint64) * np.uint64(2)
    return r


@pytest.mark.parametrize("seed", range(12))
def test_reference_against_breadth_first_search(seed):
    rng = np.random.default_rng(1200 + seed)
    n_nodes = int(rng.integers(2, 120))
    rows = _random_rows(rng, n_nodes, int(rng.integers(1, 3 * n_nodes)))
    nodes = nodes_ref(rows)
    if seed % 3 == 0 and len(nodes) > 4:                              # refs without a node row: their rows are never red
        nodes = np.delete(nodes, rng.choice(len(nodes), len(nodes) // 5, replace=False))
    trend = np.zeros(len(rows), dtype=engine.TREND_DTYPE)
    trend["lat_dev"] = rng.choice(np.array([0.0, -0.0, 1.5, 3.0, np.nan, -2.0], dtype=np.float32), len(rows))
    trend["err_dev"] = rng.standard_normal(len(rows)).astype(np.float32)
    rank = np.zeros(len(nodes), dtype=engine.RANK_DTYPE)
    rank["rank"] = rng.integers(0, 5, len(nodes)).astype(np.uint64) << np.uint64(54)   # ties, and a sum that can pass 2^56
    met = set()
    for by in ("score", "lat_dev", "err_dev"):
        val = rows["score"] if by == "score" else trend[by]
        for thr in (-INF, 0.0, quantile_threshold(val, 0.7), INF):
            for rk in (None, rank):
                got, gi = incident_ref(rows, nodes, by, thr, trend=trend, rank=rk)
                want, wi = incidents_bfs(rows, nodes, val, thr, rank=rk)
                assert got.tobytes() == want.tobytes(), (by, thr)
                assert gi.tolist() == wi.tolist()
                met.add(len(got))
            if thr == INF:
                assert len(got) == 0                                  # (no value is +inf)
    assert max(met) >= 1


def test_no_red_row_gives_no_incident():
    rows = rows_of((1, 2, 0.1), (2, 3, 0.2))
    nodes = nodes_ref(rows)
    out, inc = incident_ref(rows, nodes, "score", 0.5)
    assert len(out) == 0 and inc.tolist() == [NO] * 3
    nan = rows_of((1, 2, float("nan")))
    assert len(incident_ref(nan, nodes_ref(nan), "score", -INF)[0]) == 0       # NaN is never red, not even at -inf
    assert len(incident_ref(rows[:0], nodes[:0], "score", -INF)[0]) == 0


def test_two_disjoint_chains_are_numbered_by_their_smallest_node():
    # 5 -> 2 -> 9 and 7 -> 3 -> 8: node rows 2 3 5 7 8 9; the chain with node 2 is incident 0
    rows = rows_of((5, 2, 0.9), (2, 9, 0.8), (7, 3, 0.7), (3, 8, 0.95))
    nodes = nodes_ref(rows)
    assert nodes["ref"].tolist() == [2, 3, 5, 7, 8, 9]
    out, inc = incident_ref(rows, nodes, "score", 0.5)
    assert inc.tolist() == [0, 1, 0, 1, 1, 0]
    assert out["first_node"].tolist() == [0, 1] and out["nodes"].tolist() == [3, 3] and out["edges"].tolist() == [2, 2]
    # rows sorted: (2,9) (3,8) (5,2) (7,3): incident 0 has rows 0 and 2, incident 1 rows 1 and 3
    assert out["count"].tolist() == [10 + 12, 11 + 13] and out["err"].tolist() == [0 + 2, 1 + 3] and out["sum_ns"].tolist() == [4000, 6000]
    assert out["worst_row"].tolist() == [2, 1] and out["value_max"].tolist() == [np.float32(0.9), np.float32(0.95)]
    assert out["score_q32"].tolist() == [int(np.float64(np.float32(0.8)) * 2 ** 32) + int(np.float64(np.float32(0.9)) * 2 ** 32),
                                         int(np.float64(np.float32(0.95)) * 2 ** 32) + int(np.float64(np.float32(0.7)) * 2 ** 32)]
    assert out["culprit_node"].tolist() == [NO, NO] and out["rank_sum"].tolist() == [0, 0] and out["reserved"].tolist() == [0, 0]


def test_a_self_loop_alone_is_an_incident():
    rows = rows_of((4, 4, 0.9), (1, 2, 0.1))
    nodes = nodes_ref(rows)
    out, inc = incident_ref(rows, nodes, "score", 0.5)
    assert inc.tolist() == [NO, NO, 0]
    assert (out["nodes"][0], out["edges"][0], out["first_node"][0], out["top_node"][0], out["worst_row"][0]) == (1, 1, 2, 2, 1)


def test_a_row_that_is_not_red_joins_nothing():
    rows = rows_of((1, 2, 0.9), (2, 3, 0.1), (3, 4, 0.9))
    nodes = nodes_ref(rows)
    out, inc = incident_ref(rows, nodes, "score", 0.5)
    assert inc.tolist() == [0, 0, 1, 1] and out["edges"].tolist() == [1, 1]
    one, inc1 = incident_ref(rows, nodes, "score", 0.1)
    assert inc1.tolist() == [0] * 4 and one["edges"].tolist() == [3] and one["nodes"].tolist() == [4]


def test_a_ref_without_a_node_row_is_never_red():
    rows = rows_of((1, 2, 0.9), (2, 3, 0.9))
    nodes = nodes_ref(rows)[:2]                                       # ref 3 beyond the id spaces
    out, inc = incident_ref(rows, nodes, "score", -INF)
    assert inc.tolist() == [0, 0] and out["edges"].tolist() == [1]


def test_ties_go_to_the_smallest_index():
    rows = rows_of((1, 2, 0.5), (2, 3, 0.5), (3, 4, -0.0), (4, 5, 0.0))
    nodes = nodes_ref(rows)
    rank = rank_ref(rows, nodes)
    rank["rank"] = [7, 9, 9, 3, 9]
    out, _ = incident_ref(rows, nodes, "score", -INF, rank=rank)
    assert len(out) == 1 and out["worst_row"][0] == 0 and out["value_max"][0] == np.float32(0.5)
    assert nodes["score"].tolist()[:3] == [0.5, 0.5, 0.5] and out["top_node"][0] == 0
    assert out["culprit_node"][0] == 1 and out["rank_sum"][0] == 37
    zero = rows_of((1, 2, -0.0), (2, 3, 0.0), (3, 4, 0.0))
    z, _ = incident_ref(zero, nodes_ref(zero), "score", 0.0)          # -0.0 >= 0.0: red; +0.0 is above it, its first row wins
    assert z["edges"][0] == 3 and z["worst_row"][0] == 1 and np.signbit(z["value_max"][0]) == False  # noqa: E712
    assert z["top_node"][0] == 0                                      # (every node's score is +0.0: a side without rows has 0.0)


def test_dtype_and_struct_sizes():
    d = engine.INCIDENT_DTYPE
    assert d.itemsize == 72 and [d.fields[f][1] for f in ("count", "rank_sum", "first_node", "culprit_node", "value_max", "reserved")] == [0, 32, 40, 60, 64, 68]
    assert C.sizeof(engine.SgIncidentParams) == 16 and NO == 0xFFFFFFFF


@pytest.fixture(scope="module")
def oracle_windows(churn, oracle_lib):  # noqa: F811
    """the oracle's rows of every churn window, with nodes_ref's node rows and rank_ref's rank rows"""
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    W = weights.make_weights(2)
    out = []
    for w in wins:
        o.packed(w, labels); o.window_close(W, 2)
        rows = o.edge_rows()
        nodes = nodes_ref(rows)
        out.append((rows, nodes, rank_ref(rows, nodes, iters=3)))
    return out


def test_invariants_over_the_oracle_windows(oracle_windows):
    for rows, nodes, rank in oracle_windows:
        assert len(rows) > 1000
        for thr in [-INF, INF] + [quantile_threshold(rows["score"], q) for q in QUANTILES]:
            out, inc = incident_ref(rows, nodes, "score", thr, rank=rank)
            val, red, src, dst = red_rows(rows, nodes, "score", thr)
            assert (inc[src[red]] == inc[dst[red]]).all() and (inc[src[red]] != NO).all()   # a red row's endpoints share an incident
            assert int(out["edges"].sum()) == int(red.sum())
            flagged = np.zeros(len(nodes), bool); flagged[src[red]] = True; flagged[dst[red]] = True
            assert int(out["nodes"].sum()) == int(flagged.sum()) == int((inc != NO).sum())
            assert (np.diff(out["first_node"].astype(np.int64)) > 0).all()
            assert sum(int(x) for x in out["rank_sum"]) == sum(int(x) for x in rank["rank"][flagged])
            for i, o in enumerate(out):
                assert inc[o["first_node"]] == i == inc[o["top_node"]] == inc[o["culprit_node"]] and red[o["worst_row"]]
            if thr == INF:
                assert len(out) == 0


def test_what_the_quantile_thresholds_cover(oracle_windows):
    """QUANTILES (0, 0.5, 0.9, 0.99 of a window's scores) over the churn windows: windows of exactly one incident, windows of more
    than 3, and incidents of 3 nodes and more — what tests/test_gpu_incidents.py then meets on the device"""
    counts, big = {}, {}
    for rows, nodes, _ in oracle_windows:
        for q in QUANTILES:
            out, _ = incident_ref(rows, nodes, "score", quantile_threshold(rows["score"], q))
            counts.setdefault(q, []).append(len(out))
            big.setdefault(q, []).append(int(out["nodes"].max()) if len(out) else 0)
    flat = [c for v in counts.values() for c in v]
    assert 1 in flat, counts
    assert max(flat) > 3, counts
    assert any(c > 3 and b >= 3 for q in QUANTILES for c, b in zip(counts[q], big[q])), (counts, big)


incident_plan = plan_fixture("incident")


def _p(me, nc, slots=1, ss=16, by=0, res=0):
    return (me, nc, slots, ss, by, res)


# toy, config 2, config 3, a 2.75 M-edge / 400 k-node shard of config 5
ENGINES = [(4096, 1100), (1 << 15, 1076), (200_000, 4_500), (1_250_000, 15_000), (2_750_000, 400_000), (1, 1), (0, 0)]


def test_plan_sizes(incident_plan):
    for r in incident_plan([_p(me, nc, slots) for me, nc in ENGINES for slots in (1, 3, 8)]):
        assert r["rc"] == 0 and r["out_size"] == 72 and r["params_size"] == 16
        me, nc, slots = max(r["max_edges"], 1), max(r["ncap"], 1), r["slots"]
        assert r["threads"] == 256 and r["node_per"] % 256 == 0 and 1 <= r["node_wgs"] <= r["max_wgs"] == 1024
        assert r["node_wgs"] * r["node_per"] >= nc > (r["node_wgs"] - 1) * r["node_per"]
        assert 1 <= r["grid_wgs"] <= 1024 and 1 <= r["hook_wgs"] <= 1024 and 1 <= r["row_wgs"] <= r["max_row_wgs"] == 256
        assert r["row_wgs"] == min(r["hook_wgs"], 256)
        assert r["key_bytes"] >= 4 * nc and r["keys_bytes"] >= 24 * nc and r["stage_bytes"] >= 4 * nc and r["blk_bytes"] >= 2 * 1024 * 4
        assert r["rows_bytes"] >= 72 * nc and r["count_bytes"] >= 8 and r["node_inc_bytes"] >= 4 * nc
        for k in ("key_bytes", "keys_bytes", "blk_bytes", "stage_bytes", "rows_bytes", "count_bytes", "node_inc_bytes"):
            assert r[k] % 256 == 0
        assert r["total_bytes"] == (5 * r["key_bytes"] + r["keys_bytes"] + r["blk_bytes"] + 2 * r["stage_bytes"]
                                    + slots * (r["rows_bytes"] + r["count_bytes"] + r["node_inc_bytes"]))
        check_layout(r, {"keys": 24 * nc, **{k: 4 * nc for k in ("parent", "flag", "lab", "num", "kinc", "stage", "stage_idx", "node_inc")},
                         "blk": 2 * 1024 * 4, "rows": 72 * nc, "count": 8}, per_slot=("rows", "count", "node_inc"))
        # 52 + 76 x slots B a node key, the head counts, and 256 B of rounding for each of the 9 + 3 x slots pieces: nothing per row
        assert r["total_bytes"] <= (52 + 76 * slots) * nc + 8192 + 256 * (9 + 4 * slots)
    c3, = incident_plan([_p(1_250_000, 15_000)])
    assert (c3["node_wgs"], c3["node_per"], c3["grid_wgs"], c3["hook_wgs"], c3["row_wgs"]) == (59, 256, 59, 1024, 256) and c3["total_bytes"] < 2 << 20
    toy, = incident_plan([_p(4096, 1100)])
    assert (toy["node_wgs"], toy["grid_wgs"], toy["hook_wgs"], toy["row_wgs"]) == (5, 5, 4, 4)


def test_the_small_gpu_engine_overflows_the_rows_table(incident_plan):
    """tests/test_gpu_incidents.py: max_edges 4096 over about 8200 pods, 4096 disjoint red pairs 2i -> 2i + 1 — each of the four
    workgroups of k12_rows takes 1024 rows, each its own incident, against the 512 slots of its LDS table (K12_SLOTS; the
    engine's static_asserts tie it to the plan's kGrpIncSlots, which tests/test_group_incident_host.py reads as 512).  k12_nodes
    takes one round of 256 node rows a workgroup — 128 pairs: its table holds them"""
    r, = incident_plan([_p(4096, 8200 + 4 + 8 + 16 + 64)])
    assert (r["row_wgs"], r["node_per"]) == (4, 256) and r["grid_wgs"] * 256 >= r["ncap"]
    assert (4096 + r["row_wgs"] - 1) // r["row_wgs"] == 1024 > 512


def test_plan_parameter_checks(incident_plan):
    ok = incident_plan([_p(1000, 100, by=b) for b in (0, 1, 2)])
    assert [r["rc"] for r in ok] == [0] * 3 and [r["by"] for r in ok] == [0, 1, 2] and ok[0]["min_value"] == 0.5
    bad = incident_plan([_p(1000, 100, by=3), _p(1000, 100, by=4), _p(1000, 100, ss=12), _p(1000, 100, ss=20), _p(1000, 100, res=1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
