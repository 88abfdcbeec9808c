"""CPU tests of the workload ranking (K17): the reference tests/group_rank_ref.py against K11's reference where the map groups
nothing, against an exact-rational walk, against a hand-computed rollout chain and the weight clamp, and the plan in
alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage group_rank) — layout, sizes at config 3 and at 2^21 keys, the working
workgroups of a config-3-sized workload window and the partials' budget, parameter checks and defaults."""
import os
from fractions import Fraction

import numpy as np
import pytest

from alaz_amd import engine
from tests.group_rank_ref import group_rank_ref, group_weight, seed_sum
from tests.helpers import G
from tests.host_scaffold import contract, rank_rows_of as rows_of
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.rank_ref import M, q16, rank_ref, ref_select_rank
from tests.traces import _random_map, _random_rows

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP

# ---- under the identity map the result is K11's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_a_map_that_groups_nothing_gives_k11s_rank_rows(seed):
    """_random_rows' scores: (0, 1), 0, -0.0, negative, 1.0 and NaN; plus scores above 1 put in here"""
    rng = np.random.default_rng(1900 + seed)
    mk, ml = int(rng.integers(41, 120)), int(rng.integers(1, 20))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 5 * mk)))
    big = rng.random(len(rows)) < 0.1
    rows["score"][big] = (1.0 + 100.0 * rng.random(int(big.sum()))).astype(np.float32)
    sc = rows["score"]
    if len(rows) > 40:
        assert ((sc > 0) & (sc < 1)).any() and (sc == 0).any() and (sc >= 1).any()
    ge, gn = contract(rows, np.full(mk, NO, np.uint32), 9, mk, ml)
    nodes = nodes_ref(rows)
    assert len(ge) == len(rows) and (ge["edges"] == 1).all() and gn.tobytes() == nodes.tobytes()
    for s, e, q in zip(rows["score"], ge["edges"], ge["score_q32"]):   # (group edges of an identity map are the rows in order)
        assert group_weight(e, q) == 1 + q16(s)
    for kw in (dict(), dict(seed="uniform", iters=3), dict(iters=1, damping_q8=1), dict(iters=64, damping_q8=255, seed_min_score=0.6),
               dict(seed_min_score=1e9, iters=2)):
        assert group_rank_ref(ge, gn, **kw).tobytes() == rank_ref(rows, nodes, **kw).tobytes()


def test_identity_weights_for_every_kind_of_score():
    """floor(s * 2^32) >> 16 == floor(s * 2^16) for 0 < s < 1; s >= 1 clamps on both sides; s <= 0 and NaN add nothing"""
    vals = [0.0, -0.0, -1.0, float("nan"), 1.0, 2.0, 1e6, 0.5, 1e-9, 2.0 ** -16, 2.0 ** -17, np.float32(0.99999994), np.float32(1 / 3)]
    rows = rows_of(*[(1, 2 + i, v) for i, v in enumerate(vals)])
    ge, _ = contract(rows, [NO] * 64, 4, 64, 1)
    assert [group_weight(e, q) for e, q in zip(ge["edges"], ge["score_q32"])] == [1 + q16(s) for s in rows["score"]]
    assert [1 + q16(v) for v in (0.5, np.float32(0.99999994), 2.0 ** -17, 2.0)] == [32769, 65536, 1, 65537]


# ---- the exact-rational walk ---------------------------------------------------------------------------------------------------------
def walk(ge, gn, iters=20, D=218, seed="score", smin=0.0):
    """the walk over group edges in exact rationals WITHOUT the contract's truncations: shares"""
    pos = {int(r): v for v, r in enumerate(gn["ref"])}
    n = len(gn)
    src = [pos[int(x)] for x in ge["from_ref"]]; dst = [pos[int(x)] for x in ge["to_ref"]]
    w = [group_weight(e, q) for e, q in zip(ge["edges"], ge["score_q32"])]
    W = [0] * n
    for u, x in zip(src, w):
        W[u] += x
    a = [Fraction(q16(s)) if (seed == "score" and s >= smin) else Fraction(int(seed == "uniform")) for s in gn["score"]]
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


def _close(rk, want, iters, n, wmax):
    """The integer result against the exact walk.  Per node and iteration the truncations move: p = a * floor(M / A) less than
    A / M <= n * 2^16 * 2^-56 of the mass once; R and m (>> 8) less than 2^8 / M each; t = floor(m / W) leaves less than W at the
    node, W <= wmax (the largest out-weight) — so less than (2^9 + wmax) / M, and an error made at one node is only handed on, never
    amplified (the walk is a contraction in the 1-norm).  Summed over n nodes and iters + 1 steps it is the bound asserted; it stays
    below 1e-6 here, four orders under the shares it is held against."""
    bound = ((iters + 1) * n * (512 + wmax) + n * 65536) / M
    assert bound < 1e-6
    for got, w in zip(_shares(rk), want):
        assert abs(got - float(w)) <= bound + 1e-15                   # (1e-15: the float() of the exact share)


@pytest.mark.parametrize("seed", range(4))
def test_the_reference_follows_the_exact_walk(seed):
    rng = np.random.default_rng(2000 + seed)
    mk, ml, mg = 60, 5, 12
    rows = _random_rows(rng, mk, ml, 150)
    for gmap in (_random_map(rng, mk, mg), _random_map(rng, mk, mg, 1.0, block=7), np.zeros(mk, np.uint32)):
        ge, gn = contract(rows, gmap, mg, mk, ml)
        wmax = max(sum(group_weight(e, q) for f, e, q in zip(ge["from_ref"], ge["edges"], ge["score_q32"]) if f == u) for u in set(ge["from_ref"].tolist()))
        for kw in (dict(iters=20, D=218, seed="score"), dict(iters=5, D=131, seed="uniform")):
            rk = group_rank_ref(ge, gn, iters=kw["iters"], damping_q8=kw["D"], seed=kw["seed"])
            _close(rk, walk(ge, gn, **kw), kw["iters"], len(gn), wmax)


# ---- what it is for: a rollout chain ------------------------------------------------------------------------------------------------
def _chain(first_pod):
    """frontend (3 pods) -> checkout (2) -> payments (4) -> db (1), every pod of a tier calling every pod of the next, every row red
    with one score; pods numbered from first_pod; groups 0 .. 3"""
    sizes = (3, 2, 4, 1)
    ids, nxt = [], first_pod
    for s in sizes:
        ids.append(list(range(nxt, nxt + s))); nxt += s
    edges = [(a, b, 0.75) for up, down in zip(ids, ids[1:]) for a in up for b in down]
    gmap = np.full(64, NO, np.uint32)
    for g, tier in enumerate(ids):
        gmap[tier] = g
    return rows_of(*edges), gmap, ids


def test_rollout_chain_by_hand():
    rows, gmap, ids = _chain(0)
    ge, gn = contract(rows, gmap, 8, 64, 1)
    assert gn["ref"].tolist() == [G(0), G(1), G(2), G(3)] and ge["edges"].tolist() == [6, 8, 4]
    assert len(set(gn["score"].tolist())) == 1                         # the four workload scores tie: the score cannot name the cause
    q = q16(0.75)
    assert [group_weight(e, s) for e, s in zip(ge["edges"], ge["score_q32"])] == [6 * (1 + q), 8 * (1 + q), 4 * (1 + q)]
    for seed in ("score", "uniform"):
        rk = group_rank_ref(ge, gn, seed=seed)
        sh = _shares(rk)
        assert ref_select_rank(rk, 1).tolist() == [3] and sh[3] == max(sh)   # db, where the red stops
        # a chain with one out edge per workload hands everything on: after k >= 3 iterations with p = 1/4 each and d = D / 256,
        # frontend keeps (1 - d) / 4, checkout (1 - d)(1 + d) / 4, payments (1 - d)(1 + d + d^2) / 4, db the rest
        d = Fraction(218, 256)
        want = [(1 - d) / 4, (1 - d) * (1 + d) / 4, (1 - d) * (1 + d + d * d) / 4]
        want.append(1 - sum(want))
        for got, w in zip(sh, want):
            assert abs(got - float(w)) < 1e-9
    # the same services after a rollout (new pods, same groups): the same rank rows, byte for byte
    rows2, gmap2, _ = _chain(20)
    ge2, gn2 = contract(rows2, gmap2, 8, 64, 1)
    assert group_rank_ref(ge2, gn2).tobytes() == group_rank_ref(ge, gn).tobytes()
    # K11 over the pods names a pod, and another one after the rollout
    before, after = rank_ref(rows, nodes_ref(rows)), rank_ref(rows2, nodes_ref(rows2))
    assert before["ref"][ref_select_rank(before, 1)[0]] != after["ref"][ref_select_rank(after, 1)[0]]


def test_pod_ranks_summed_per_owner_are_a_different_walk():
    """replicas without an anomalous out-row hold the mass in pod space: summing K11's pod ranks per owner is not this ranking"""
    a, b1, b2, b3, b4, c = range(6)
    rows = rows_of((a, b1, 0.9), (a, b2, 0.9), (a, b3, 0.9), (a, b4, 0.9), (b1, c, 0.9))   # of b's four replicas only b1 calls c this window
    gmap = np.array([0, 1, 1, 1, 1, 2] + [NO] * 2, np.uint32)
    ge, gn = contract(rows, gmap, 4, 8, 1)
    rk = group_rank_ref(ge, gn)
    pods = rank_ref(rows, nodes_ref(rows))
    owner_sum = [int(pods["rank"][0]), sum(int(x) for x in pods["rank"][1:5]), int(pods["rank"][5])]
    assert ref_select_rank(rk, 1).tolist() == [2]                      # the workload walk: c, the sink
    assert owner_sum.index(max(owner_sum)) == 1                        # the summed pod walk: b, three of whose pods are sinks there


# ---- the weight clamp, and group edges without a key ---------------------------------------------------------------------------------
def test_weight_clamp():
    assert group_weight(1, 5 << 32) == 65537 and group_weight(3, (3 << 32) + 12345) == 3 * 65537
    assert group_weight(2, 1 << 32) == 2 + 65536 and group_weight(2, 0) == 2 and group_weight(4, 0xFFFF) == 4
    rows = rows_of((0, 2, 7.5), (1, 2, 0.25))                         # one group edge: scores 7.5 and .25 fold to 7.75 x 2^32
    ge, gn = contract(rows, [0, 0, NO, NO], 2, 4, 1)
    assert len(ge) == 1 and int(ge["score_q32"][0]) >> 16 > 65536 * int(ge["edges"][0]) == 131072
    assert group_weight(ge["edges"][0], ge["score_q32"][0]) == 2 * 65537 > (1 + q16(7.5)) + (1 + q16(0.25))
    group_rank_ref(ge, gn)                                             # (its asserts hold: w <= 65537 * edges)


def test_a_group_edge_without_a_key_carries_nothing():
    rows = rows_of((0, 1, 0.5), (1, 2, 0.5))
    ge, gn = contract(rows, [NO] * 4, 2, 4, 1)
    full = group_rank_ref(ge, gn, iters=3)
    cut = group_rank_ref(ge, gn, iters=3, no_key={2})
    assert full.tobytes() != cut.tobytes() and int(cut["rank"][1]) > int(full["rank"][1])   # node 1 is a sink once 1 -> 2 is cut


def test_seed_fallback_and_empty_window():
    rows = rows_of((0, 1, 0.5), (1, 2, 0.25))
    ge, gn = contract(rows, [NO] * 4, 2, 4, 1)
    assert seed_sum(gn, seed_min_score=0.75) == 0 and seed_sum(gn) > 0 and seed_sum(gn, "uniform") == 3
    assert group_rank_ref(ge, gn, seed_min_score=0.75).tobytes() == group_rank_ref(ge, gn, seed="uniform").tobytes()
    assert len(group_rank_ref(ge[:0], gn[:0])) == 0


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("group_rank")


def _p(me, ncap, mg, slots=1, rows=0, ss=24, iters=0, damp=0, seed=0, res=0):
    return (me, ncap, mg, slots, rows, ss, iters, damp, seed, res)


NR = 8192
# toy, config 2, config 3 (15 k node ids, as many groups), K16's 2^21-key limit, degenerate
ENGINES = [(4096, 1100, 1000), (1 << 15, 1076, 1076), (1_250_000, 15_000, 15_000), (2_750_000, 400_000, 100_000),
           (4_000_000, 1 << 20, 1 << 20), (1, 1, 1), (0, 0, 0)]


def test_plan_sizes_and_layout(plan):
    for r in plan([_p(me, nc, mg, slots) for me, nc, mg in ENGINES for slots in (1, 3, 8)]):
        assert r["rc"] == 0 and r["rank_size"] == 16 and r["params_size"] == 24
        me, slots = max(r["max_edges"], 1), r["slots"]
        gk, nc = max(r["gk"], 1), max(r["nc"], 1)
        assert r["gk"] == r["ncap"] + r["max_groups"] and r["nc"] == min(gk, 2 * me)
        assert r["range_rows"] == NR and r["ranges"] * NR >= nc > (r["ranges"] - 1) * NR
        assert 2 * r["lds_bytes"] == 2 * NR * 8 <= r["lds_limit"] == 160 * 1024     # two workgroups a CU
        assert 1 <= r["slices"] <= r["max_slices"] == 256 and r["slices"] <= max(1, -(-me // r["slice_edges"]))
        assert r["ranges"] * r["slices"] * NR * 8 <= r["part_budget"] == 128 << 20 or r["slices"] == 1
        assert 1 <= r["pos_wgs"] <= r["max_wgs"] == 1024 and 1 <= r["prep_wgs"] <= 1024 and 1 <= r["node_wgs"] <= 1024
        need = {"pos": 4 * gk, "src": 4 * me, "dst": 4 * me, "w": 8 * me, **{k: 8 * nc for k in ("W", "R", "base", "t")}, "rows": 16 * nc,
                "stage": 16 * nc, "stage_idx": 4 * nc, "seed": 8 * r["max_wgs"], "part": r["ranges"] * r["slices"] * NR * 8}
        check_layout(r, need, per_slot=("rows",))
        assert r["part_bytes"] == need["part"] and r["total_bytes"] <= sum(need.values()) + (slots - 1) * 16 * nc + 256 * (12 + slots)
        assert r["live_wgs"] == 0                                      # (a window without rows: every workgroup exits)


def test_plan_at_config_3_and_at_the_key_limit(plan):
    # config 3's workload window as the probe makes it: 590 k group edges, about 5.6 k workload rows — ONE live range, one slice per
    # CU of a 256-CU part, where K11's plan has 32 workgroups
    c3, = plan([_p(1_250_000, 15_000, 15_000, rows=5_600)])
    assert (c3["ranges"], c3["slices"], c3["live_wgs"]) == (4, 256, 256)
    assert c3["part_bytes"] == 4 * 256 * NR * 8 == 64 << 20 and c3["total_bytes"] < 90 << 20
    per = -(-590_000 // c3["slices"])
    assert per == 2305 <= 1024 * 4                                     # a slice's group edges: under one trip of the workgroup
    full, = plan([_p(1_250_000, 15_000, 15_000, rows=30_000)])
    assert full["live_wgs"] == 4 * 256                                  # every row of the slot in use: every range works
    # K16's limit: 2^21 keys, 256 ranges; the budget leaves 8 slices and the partials are exactly 128 MiB
    lim, = plan([_p(4_000_000, 1 << 20, 1 << 20, rows=1 << 21)])
    assert (lim["gk"], lim["nc"], lim["ranges"], lim["slices"]) == (1 << 21, 1 << 21, 256, 8)
    assert lim["part_bytes"] == 128 << 20 and lim["live_wgs"] == 2048 and lim["total_bytes"] < 336 << 20
    small, = plan([_p(4_000_000, 1 << 20, 1 << 20, rows=5_600)])
    assert small["live_wgs"] == 8                                       # (the budget's price: few slices on a big engine's small window)
    toy, = plan([_p(4096, 1100, 1000, rows=NR + 1)])
    assert (toy["ranges"], toy["slices"], toy["pos_wgs"], toy["prep_wgs"], toy["node_wgs"], toy["live_wgs"]) == (1, 2, 9, 4, 66, 2)
    assert c3["node_wgs"] == -(-30_000 // 32) and lim["node_wgs"] == 1024   # blocks of 32 rows, at most 1024 workgroups


def test_plan_defaults_and_invalid_parameters(plan):
    d, = plan([_p(1000, 100, 10)])
    assert (d["iters"], d["damping_q8"], d["seed"]) == (20, 218, 0)
    k, = plan([_p(1000, 100, 10, iters=64, damp=255, seed=1)])
    assert (k["iters"], k["damping_q8"], k["seed"]) == (64, 255, 1)
    bad = plan([_p(1000, 100, 10, iters=65), _p(1000, 100, 10, damp=256), _p(1000, 100, 10, seed=2), _p(1000, 100, 10, ss=20),
                _p(1000, 100, 10, ss=28), _p(1000, 100, 10, res=1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 6
