"""CPU tests of the culprit ranking (K11): the reference tests/rank_ref.py against hand-worked cases that pin what the ranking
means, the selection's reference, and the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage rank) — sizes for every
engine, parameter checks and defaults."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.host_scaffold import rank_rows_of as rows_of
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.rank_ref import M, q16, rank_keys, rank_ref, ref_select_rank

HERE = os.path.dirname(os.path.abspath(__file__))
FE, CART, PAY, DB, CAT, DB2 = range(1, 7)                            # KNOWN refs (type 0): the ref is the id


def walk(rows, nodes, iters=20, D=218, seed="score", smin=0.0):
    """the same walk in exact rationals WITHOUT the contract's truncations (an independent statement of the definition): shares"""
    pos = {int(r): v for v, r in enumerate(nodes["ref"])}
    n = len(nodes)
    src = [pos[int(x)] for x in rows["from_ref"]]; dst = [pos[int(x)] for x in rows["to_ref"]]
    w = [1 + q16(s) for s in rows["score"]]
    W = [0] * n
    for u, x in zip(src, w):
        W[u] += x
    a = [Fraction(q16(s)) if (seed == "score" and s >= smin) else Fraction(int(seed == "uniform")) for s in nodes["score"]]
    if sum(a) == 0:
        a = [Fraction(1)] * n
    p = [x / sum(a) for x in a]
    d = Fraction(D, 256)
    r = list(p)
    for _ in range(iters):
        nr = [(1 - d) * pv + (d * rv if Wv == 0 else 0) for pv, rv, Wv in zip(p, r, W)]
        for u, v, x in zip(src, dst, w):
            nr[v] += d * r[u] * x / W[u]
        r = nr
    assert sum(r) == 1
    return r


def _shares(rk):
    return [int(x) / M for x in rk["rank"]]


def _close(rk, want, iters, n):
    """the integer result against the exact walk: every truncation (p, R, m: >> 8; t: the division, kept at the node) moves less
    than 2^-40 of the mass per node and iteration, far below the 1e-9 asserted"""
    assert (iters + 2) * n * 2.0 ** -40 < 1e-9
    for got, w in zip(_shares(rk), want):
        assert abs(got - float(w)) < 1e-9


def test_dtype_and_struct_sizes():
    assert engine.RANK_DTYPE.itemsize == 16 and [engine.RANK_DTYPE.fields[f][1] for f in ("rank", "ref", "share")] == [0, 8, 12]
    assert C.sizeof(engine.SgRankParams) == 24
    assert engine.RANK_SEED == dict(score=0, uniform=1)


def test_q16():
    assert [q16(x) for x in (0.0, -1.0, float("nan"), 1.0, 2.0, 0.5, 1e-9)] == [0, 0, 0, 65536, 65536, 32768, 0]
    assert q16(np.float32(0.99999994)) == 65535


def test_two_nodes_closed_form():
    """a -> b, uniform seed: a hands everything on, so after any iteration a holds its restart (1 - d) / 2 and b the rest,
    (1 + d) / 2: with D = 218 the ratio b / a is 474 / 38"""
    rows = rows_of((1, 2, 0.25))
    nodes = nodes_ref(rows)
    for iters in (1, 20, 64):
        rk = rank_ref(rows, nodes, iters=iters, seed="uniform")
        sa, sb = _shares(rk)
        assert abs(sa - 38 / 512) < 1e-12 and abs(sb - 474 / 512) < 1e-12
        assert int(rk["rank"].sum()) <= M and M - int(rk["rank"].sum()) < 1 << 20
    assert rk["ref"].tolist() == [1, 2] and rk["share"][1] == np.float32(int(rk["rank"][1]) * 2.0 ** -56)


def test_red_chain_beside_a_healthy_branch_names_the_sink():
    """fe -> cart -> pay -> db red (.8 / .85 / .9) beside a healthy fe -> cat -> db2: db, where the red stops, is first under both
    seeds, and ahead of the second by the factor the exact walk gives"""
    rows = rows_of((FE, CART, 0.8), (CART, PAY, 0.85), (PAY, DB, 0.9), (FE, CAT, 0.02), (CAT, DB2, 0.02))
    nodes = nodes_ref(rows)
    assert nodes["ref"].tolist() == [FE, CART, PAY, DB, CAT, DB2]
    for seed in ("score", "uniform"):
        rk = rank_ref(rows, nodes, seed=seed)
        want = walk(rows, nodes, seed=seed)
        _close(rk, want, 20, 6)
        order = ref_select_rank(rk, 6)
        assert order[0] == 3, (seed, _shares(rk))                     # db
        second = sorted(want, reverse=True)[1]
        factor = float(want[3] / second)
        assert factor > 1.5
        got = _shares(rk)
        assert abs(got[3] / got[order[1]] - factor) < 1e-6
        assert got[3] > got[5]                                         # the healthy branch's sink is behind
    # the three red callers have nearly one node score; the ranking separates them from the cause
    sc = rank_ref(rows, nodes)
    assert _shares(sc)[3] > 5 * max(_shares(sc)[i] for i in (0, 1, 2))


def test_a_sink_without_anomaly_does_not_outrank_the_red_sink():
    """two sinks behind one caller, equal traffic: x red (.9), y healthy (.01) — under the score seed x is first by the exact
    walk's factor; the healthy sink keeps only what the +1 of the weights and its own small seed give it"""
    rows = rows_of((1, 2, 0.9), (1, 3, 0.01))
    nodes = nodes_ref(rows)
    rk = rank_ref(rows, nodes)
    want = walk(rows, nodes)
    _close(rk, want, 20, 3)
    s = _shares(rk)
    assert ref_select_rank(rk, 1).tolist() == [1]
    assert s[1] > s[2] and abs(s[1] / s[2] - float(want[1] / want[2])) < 1e-6 and want[1] / want[2] > 20


def test_self_loop_and_pure_source():
    """b calls itself (an ordinary row: mass that takes it comes back to b) and c; a is only a source: it keeps its restart only"""
    rows = rows_of((1, 2, 0.5), (2, 2, 0.5), (2, 3, 0.5))
    nodes = nodes_ref(rows)
    for seed in ("score", "uniform"):
        tr = []
        rk = rank_ref(rows, nodes, seed=seed, trace=tr)
        want = walk(rows, nodes, seed=seed)
        _close(rk, want, 20, 3)
        p0 = walk(rows, nodes, iters=0, seed=seed)[0]
        assert abs(_shares(rk)[0] - float(p0 * Fraction(38, 256))) < 1e-9   # a: (1 - d) p_a and nothing else
        assert ref_select_rank(rk, 1).tolist() == [2]                  # c, the sink
        assert len(tr) == 20


def test_zero_seed_falls_back_to_uniform():
    rows = rows_of((1, 2, 0.0), (2, 3, -0.0))
    nodes = nodes_ref(rows)
    assert rank_ref(rows, nodes).tobytes() == rank_ref(rows, nodes, seed="uniform").tobytes()
    hi = rows_of((1, 2, 0.5), (2, 3, 0.25))
    n2 = nodes_ref(hi)
    assert rank_ref(hi, n2, seed_min_score=0.75).tobytes() == rank_ref(hi, n2, seed="uniform").tobytes()    # every node below it
    only = rank_ref(hi, n2, seed_min_score=0.5)                       # node 3 (score .25) seeds nothing
    assert _shares(only)[2] > 0 and only.tobytes() != rank_ref(hi, n2).tobytes()


def test_one_node_keeps_all_the_mass_and_its_key_is_clamped():
    rows = rows_of((7, 7, 0.5))
    nodes = nodes_ref(rows)
    for iters in (1, 64):
        rk = rank_ref(rows, nodes, iters=iters)
        # A = q16(.5) = 2^15 divides M: p = M; the self-loop hands floor(m / W) * W back and the rest stays
        assert int(rk["rank"][0]) == (M >> 8) * 38 + (M >> 8) * 218 == M
        assert rk["share"][0] == 1.0
    assert int(rank_keys(rk)[0]) == 0xFFFFFFFF and (M >> 24) == 1 << 32
    assert ref_select_rank(rk, 1).tolist() == [0]


def test_hub_with_60000_out_rows_of_score_one():
    """the largest W the contract meets per row count: 60 000 x 65 537; t = m / W is small, what the division leaves stays at the
    hub, nothing overflows (the reference asserts every product and the mass on every iteration)"""
    n = 60_000
    rows = np.zeros(n, dtype=EDGE_OUT_DTYPE)
    rows["from_ref"] = 1; rows["to_ref"] = np.arange(2, n + 2); rows["score"] = 1.0; rows["count"] = 1
    nodes = nodes_ref(rows)
    tr = []
    rk = rank_ref(rows, nodes, iters=3, trace=tr)
    W = n * 65537
    p_hub = int(q16(1.0)) * (M // ((n + 1) * 65536))
    m0 = (p_hub >> 8) * 218
    assert tr[0][0] == (p_hub >> 8) * 38 + m0 % W                      # the hub after one iteration: restart + the remainder
    assert int(rk["rank"].sum()) <= M and M - int(rk["rank"].sum()) < 1 << 36   # A < 2^33 of p, 2^16 a node and iteration
    assert (rank_keys(rk) > 0).all()


@pytest.mark.parametrize("iters", [1, 64])
@pytest.mark.parametrize("D", [1, 255])
def test_extreme_iterations_and_damping(iters, D):
    rows = rows_of((FE, CART, 0.8), (CART, PAY, 0.85), (PAY, DB, 0.9), (FE, CAT, 0.02), (CAT, DB2, 0.02), (DB, DB, 0.3))
    nodes = nodes_ref(rows)
    rk = rank_ref(rows, nodes, iters=iters, damping_q8=D)
    _close(rk, walk(rows, nodes, iters=iters, D=D), iters, 6)
    if D == 1:                                                         # almost all restart: the ranking is the seed's
        a = np.array([q16(s) for s in nodes["score"]], dtype=np.float64)
        assert np.abs(np.array(_shares(rk)) - a / a.sum()).max() < 1 / 64
    else:                                                              # almost no restart: after 64 steps everything sits at the sink
        assert (_shares(rk)[3] > 0.95) == (iters == 64)


def test_selection_reference():
    rk = np.zeros(6, engine.RANK_DTYPE)
    rk["rank"] = [5 << 24, 9 << 24, (1 << 24) - 1, 9 << 24, M, 5 << 24]
    rk["share"] = (rk["rank"].astype(np.float64) * 2.0 ** -56).astype(np.float32)
    assert ref_select_rank(rk, 0).tolist() == [0, 1, 3, 4, 5]          # key 0 (rank < 2^24) is no candidate
    assert ref_select_rank(rk, 4).tolist() == [4, 1, 3, 0]             # ties by position
    assert ref_select_rank(rk, 100).tolist() == [4, 1, 3, 0, 5]
    assert ref_select_rank(rk, 0, float(rk["share"][1])).tolist() == [1, 3, 4]
    assert ref_select_rank(rk, 2, float("nan")).tolist() == []


rank_plan = plan_fixture("rank")


def _p(me, nc, slots=1, ss=24, iters=0, damp=0, seed=0, res=0):
    return (me, nc, slots, ss, iters, damp, seed, res)


# toy, config 2, config 3, a 2.75 M-edge / 400 k-node shard of config 5
ENGINES = [(4096, 1100), (1 << 15, 1076), (200_000, 4_500), (1_250_000, 15_000), (2_750_000, 400_000), (1, 1), (0, 0)]


def test_plan_sizes(rank_plan):
    for r in rank_plan([_p(me, nc, slots) for me, nc in ENGINES for slots in (1, 3, 8)]):
        assert r["rc"] == 0 and r["rank_size"] == 16 and r["params_size"] == 24
        me, nc, slots = max(r["max_edges"], 1), max(r["ncap"], 1), r["slots"]
        assert r["range_nodes"] == 16384 and r["ranges"] * 16384 >= nc > (r["ranges"] - 1) * 16384
        assert r["lds_bytes"] == 16384 * 8 <= r["lds_limit"] == 160 * 1024
        assert 1 <= r["slices"] <= 32 and (r["ranges"] * r["slices"] <= r["max_edge_wgs"] == 256 or r["slices"] == 1)
        assert 1 <= r["prep_wgs"] <= r["max_wgs"] == 1024 and 1 <= r["node_wgs"] <= 1024
        assert r["row_bytes"] >= 4 * me and r["node_bytes"] >= 8 * nc and r["rows_bytes"] >= 16 * nc and r["stage_bytes"] >= 16 * nc
        assert r["stage_idx_bytes"] >= 4 * nc and r["seed_bytes"] >= 8 * r["max_wgs"]
        assert r["part_bytes"] >= r["ranges"] * r["slices"] * 16384 * 8
        for k in ("row_bytes", "node_bytes", "rows_bytes", "stage_bytes", "stage_idx_bytes", "seed_bytes", "part_bytes"):
            assert r[k] % 256 == 0
        assert r["total_bytes"] == (3 * r["row_bytes"] + 4 * r["node_bytes"] + r["part_bytes"] + r["seed_bytes"] + r["stage_bytes"]
                                    + r["stage_idx_bytes"] + slots * r["rows_bytes"])
        check_layout(r, {**{k: 4 * me for k in ("src", "dst", "w")}, **{k: 8 * nc for k in ("W", "R", "base", "t")}, "rows": 16 * nc,
                         "stage": 16 * nc, "stage_idx": 4 * nc, "seed": 8 * r["max_wgs"], "part": r["ranges"] * r["slices"] * 16384 * 8},
                     per_slot=("rows",))
        # 12 B a row, 32 + 20 + 16 x slots B a node key, the partials (at most 256 workgroups x 128 KiB, or one slice per range),
        # the seed sums, and 256 B of rounding for each of the 11 + slots pieces
        assert r["total_bytes"] <= 12 * me + (52 + 16 * slots) * nc + max(256, r["ranges"]) * 16384 * 8 + 8192 + 256 * (11 + slots)
    c3, = rank_plan([_p(1_250_000, 15_000)])
    assert (c3["ranges"], c3["slices"]) == (1, 32) and c3["total_bytes"] < 21 << 20    # config 3: ONE node range
    c5, = rank_plan([_p(2_750_000, 400_000)])
    assert (c5["ranges"], c5["slices"]) == (25, 10) and c5["total_bytes"] < 96 << 20
    toy, = rank_plan([_p(4096, 1100)])
    assert (toy["ranges"], toy["slices"], toy["prep_wgs"], toy["node_wgs"]) == (1, 1, 4, 5)


def test_plan_defaults_and_invalid_parameters(rank_plan):
    d, = rank_plan([_p(1000, 100)])
    assert (d["iters"], d["damping_q8"], d["seed"]) == (20, 218, 0)
    k, = rank_plan([_p(1000, 100, iters=64, damp=255, seed=1)])
    assert (k["iters"], k["damping_q8"], k["seed"]) == (64, 255, 1)
    k, = rank_plan([_p(1000, 100, iters=1, damp=1)])
    assert (k["iters"], k["damping_q8"]) == (1, 1)
    bad = rank_plan([_p(1000, 100, iters=65), _p(1000, 100, damp=256), _p(1000, 100, seed=2), _p(1000, 100, ss=20), _p(1000, 100, ss=28),
                     _p(1000, 100, res=1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 6
