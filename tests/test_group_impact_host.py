"""CPU tests of the workload impact (K22): the reference tests/impact_ref.py against a second statement of the contract written
apart from it (distances by repeated boolean matrix products) over random windows made with the existing references, hand cases,
the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage group_impact) — layout, sizes at config 3 and at 2^21 keys,
parameter checks — and the header's constants against engine.py."""
import os
import subprocess

import numpy as np
import pytest

from alaz_amd import engine
from tests.group_incident_ref import group_incident_ref
from tests.helpers import G
from tests.host_scaffold import contract, incident_rows_of as rows_of
from tests.impact_ref import call_edges, impact_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.traces import _random_map, _random_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NO = engine.NO_INCIDENT
NOH = engine.NO_HOPS
U64 = (1 << 64) - 1
(EXPOSED, DIRECT, FAR, ENTRIES, ENTRY_COUNT, ENTRY_ERR, INTO_COUNT, INTO_ERR) = range(8)


def impact_matrix(ge, gn, n_inc, inc, max_incidents, max_hops):
    """the contract again, on its own: A[u, v] = "u calls v" as a boolean matrix; the rows within r call edges of incident i's
    members are R_r = R_(r-1) | A @ R_(r-1), and d_i(x) is the first r at which x appears"""
    n = len(gn)
    at = {int(r): v for v, r in enumerate(gn["ref"])}
    A = np.zeros((n, n), dtype=bool)
    cnt = np.zeros((n, n), dtype=object); err = np.zeros((n, n), dtype=object)
    for j in range(len(ge)):
        u, v = at.get(int(ge["from_ref"][j])), at.get(int(ge["to_ref"][j]))
        if u is None or v is None or u == v or int(ge["count"][j]) == 0:
            continue
        A[u, v] = True
        cnt[u, v] += int(ge["count"][j]); err[u, v] += int(ge["err_count"][j])
    entry = ~A.any(axis=0)
    inc = np.asarray(inc, dtype=np.int64)
    cov = min(n_inc, max_incidents)
    W = (max_incidents + 63) // 64
    rows = np.zeros((cov, 8), dtype="<u8")
    dist = np.full((cov, n), -1, dtype=np.int64)
    for i in range(cov):
        reach = inc == i
        dist[i, reach] = 0
        for r in range(1, max_hops + 1):
            grown = reach | (A.astype(np.uint8) @ reach.astype(np.uint8) > 0)
            dist[i, grown & ~reach] = r
            reach = grown
        d = dist[i]
        ex = np.flatnonzero(d >= 1)
        far = 0xFFFFFFFF if not len(ex) else int(d[ex].max()) << 32 | int(ex[d[ex] == d[ex].max()].min())
        ent = np.flatnonzero((d >= 0) & entry)
        member = inc == i
        into = A & member[None, :] & ~member[:, None]
        rows[i] = [len(ex), int((d == 1).sum()), far, len(ent), sum(int(x) for x in gn["out_count"][ent]) & U64,
                   sum(int(x) for x in gn["out_err"][ent]) & U64, int(sum(cnt[into])) & U64 if into.any() else 0,
                   int(sum(err[into])) & U64 if into.any() else 0]
    hops = np.full(n, NOH, dtype="<u4")
    mask = np.zeros((n, W), dtype="<u8")
    for v in range(n):
        ds = [int(dist[i, v]) for i in range(cov) if dist[i, v] >= 0]
        if ds:
            hops[v] = min(ds)
        for i in range(cov):
            if dist[i, v] >= 0:
                mask[v, i >> 6] |= np.uint64(1 << (i & 63))
    return rows, hops, mask


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _random_window(rng):
    mk, ml, mg = int(rng.integers(4, 60)), int(rng.integers(1, 8)), int(rng.integers(1, 16))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 3 * mk)))
    gmap = _random_map(rng, mk, mg, share=float(rng.choice([0.0, 0.5, 1.0])), block=(None, 3)[int(rng.integers(0, 2))])
    ge, gn = contract(rows, gmap, mg, mk, ml)
    ge["score_max"] = rng.random(len(ge)).astype(np.float32)
    for f in ("count", "err_count"):
        ge[f] = rng.integers(0, 1 << 63, len(ge), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(ge)).astype(np.uint64)
    ge["count"][rng.random(len(ge)) < 0.15] = 0                         # alive-only group edges
    for f in ("out_count", "out_err"):
        gn[f] = rng.integers(0, 1 << 63, len(gn), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(gn)).astype(np.uint64)
    return ge, gn


@pytest.mark.parametrize("block", range(4))
def test_reference_against_matrix_products(block):
    """200 seeds, 50 a case, rows <= 200; thresholds from "every group edge red" to "a few", parameters that cover all, some and one
    incident and cut the search"""
    seen_cut, seen_uncovered, seen_far = 0, 0, 0
    for seed in range(50 * block, 50 * block + 50):
        rng = np.random.default_rng(2200 + seed)
        ge, gn = _random_window(rng)
        assert len(gn) <= 200
        if seed % 4 == 0 and len(gn) > 4:                             # refs without a workload row: no call edge
            gn = np.delete(gn, rng.choice(len(gn), len(gn) // 6, replace=False))
        thr = float(rng.choice([0.0, 0.5, 0.8, 0.95]))
        incs, inc = group_incident_ref(ge, gn, "score", thr)
        for mi, mh in ((int(rng.integers(1, 6)), int(rng.integers(1, 4))), (64, 64), (65, 2), (1024, 8)):
            want = impact_matrix(ge, gn, len(incs), inc, mi, mh)
            got = impact_ref(ge, gn, len(incs), inc, mi, mh)
            _same(got, want)
            seen_uncovered += len(incs) > mi
            seen_cut += int((got[0][:, FAR] >> np.uint64(32) == mh).sum()) if len(got[0]) else 0
            seen_far += int((got[0][:, FAR] >> np.uint64(32) >= 2).sum()) if len(got[0]) else 0
    assert seen_cut and seen_uncovered and seen_far


def _hand(edges, red, max_incidents=8, max_hops=8, mk=16, counts=None, gmap=None):
    """rows from (from, to) pod pairs; `red` of them get score 1, the others 0; incidents at 0.5"""
    rows = rows_of(*[(f, t, 1.0 if (f, t) in red else 0.0) for f, t in edges])
    if counts:
        for i, (f, t) in enumerate(sorted(edges)):
            if (f, t) in counts:
                rows[i]["count"] = counts[(f, t)]
    gmap = np.full(mk, engine.NO_GROUP, np.uint32) if gmap is None else gmap
    ge, gn = contract(rows, gmap, mk, mk, 4)
    incs, inc = group_incident_ref(ge, gn, "score", 0.5)
    return ge, gn, incs, inc, impact_ref(ge, gn, len(incs), inc, max_incidents, max_hops)


def test_a_chain_both_ways_and_cut():
    up = [(i, i + 1) for i in range(12)]                              # 0 -> 1 -> ... -> 12, the last edge red
    for edges, red, order in ((up, {(11, 12)}, lambda v: 11 - v), ([(b, a) for a, b in up], {(1, 0)}, lambda v: v - 1)):
        for mh in (11, 12, 4):
            ge, gn, incs, inc, (rows, hops, mask) = _hand(edges, red, max_hops=mh)
            assert len(incs) == 1 and len(gn) == 13
            members = set(np.flatnonzero(inc == 0).tolist())
            d = [0 if v in members else order(v) for v in range(13)]
            assert hops.tolist() == [x if x <= mh else NOH for x in d]
            assert rows[0, EXPOSED] == min(11, mh) and rows[0, DIRECT] == 1
            assert rows[0, FAR] >> np.uint64(32) == min(11, mh)
            assert rows[0, ENTRIES] == (1 if mh >= 11 else 0)
            assert (mask[:, 0] != 0).tolist() == [x <= mh for x in d]


def test_a_diamond_a_cycle_and_the_edge_kinds():
    # 0 -> 9 (red 9 -> 10); 0 -> 1 -> 2 -> 9: the shorter path wins
    _, _, _, _, (rows, hops, _) = _hand([(0, 9), (0, 1), (1, 2), (2, 9), (9, 10)], {(9, 10)})
    assert hops.tolist()[:3] == [1, 2, 1] and rows[0].tolist()[:2] == [3, 2]
    # a 3-cycle through a member: 0 -> 1 -> 2 -> 0, red 0 -> 5
    _, _, _, inc, (rows, hops, _) = _hand([(0, 1), (1, 2), (2, 0), (0, 5)], {(0, 5)})
    assert hops.tolist() == [0, 2, 1, 0] and rows[0, EXPOSED] == 2 and rows[0, ENTRIES] == 0
    # an alive-only edge 3 -> 0 and traffic inside the workload {0, 1} expose nobody; 4 calls itself and 0: still an entry
    gmap = np.full(16, engine.NO_GROUP, np.uint32); gmap[[0, 1]] = 7
    ge, gn, incs, inc, (rows, hops, _) = _hand([(0, 5), (1, 0), (3, 0), (4, 4), (4, 0)], {(0, 5)}, counts={(3, 0): 0}, gmap=gmap)
    ref = {int(r): v for v, r in enumerate(gn["ref"])}
    assert hops[ref[3]] == NOH and hops[ref[4]] == 1 and hops[ref[G(7)]] == 0
    assert rows[0, EXPOSED] == 1 and rows[0, ENTRIES] == 1 and rows[0, ENTRY_COUNT] == int(gn["out_count"][ref[4]])
    into = [(c, e) for u, v, c, e in call_edges(ge, gn) if u == ref[4] and v == ref[G(7)]]
    assert rows[0, INTO_COUNT] == into[0][0] and rows[0, INTO_ERR] == into[0][1]


def test_word_boundaries_and_uncovered_incidents():
    """129 single-edge incidents 2i -> 2i + 1, each with its own caller 300 + i, and row 299 calling a member of every incident"""
    n = 129
    edges = [(2 * i, 2 * i + 1) for i in range(n)] + [(300 + i, 2 * i) for i in range(n)] + [(299, 2 * i) for i in range(n)]
    red = {(2 * i, 2 * i + 1) for i in range(n)}
    for mi in (1, 64, 65, 100, 129, 200):
        ge, gn, incs, inc, (rows, hops, mask) = _hand(edges, red, max_incidents=mi, mk=512)
        assert len(incs) == n and len(rows) == min(n, mi) and mask.shape[1] == (mi + 63) // 64
        ref = {int(r): v for v, r in enumerate(gn["ref"])}
        bits = sum(int(mask[ref[299], w]) << (64 * w) for w in range(mask.shape[1]))
        assert bits == (1 << min(n, mi)) - 1                          # bits of uncovered incidents are 0
        assert (rows[:, EXPOSED] == 2).all() and (rows[:, DIRECT] == 2).all() and (rows[:, ENTRIES] == 2).all()
        assert [int(hops[ref[300 + i]]) for i in range(n)] == [1 if i < mi else NOH for i in range(n)]


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("group_impact")


ENGINES = [(1 << 14, 300, 300), (4096, 8192 + 88, 8192 + 8), (1_250_000, 15_000, 15_000), (0, 0, 0), (1000, 50, 1 << 20)]


def test_plan_sizes_and_layout(plan):
    for r in plan([(me, nc, mg, slots, mi, 8) for me, nc, mg in ENGINES for slots in (1, 3, 8) for mi in (1, 64, 65, 256, 1024)]):
        assert r["rc"] == 0 and r["impact_words"] == 8 and r["launches"] == 20
        me, gk, nc, mi = max(r["max_edges"], 1), max(r["gk"], 1), max(r["nc"], 1), r["max_incidents"]
        W = -(-mi // 64)
        assert r["words"] == W and r["threads"] == 256 and r["max_wgs"] == 1024
        assert r["node_wgs"] == max(1, min(1024, -(-nc // 256))) and r["edge_wgs"] == max(1, min(1024, -(-me // 1024)))
        assert r["finish_wgs"] * 256 >= mi
        need = {"pos": 4 * gk, "fresh": 8 * W * nc, "next": 8 * W * nc, "mask": 8 * W * nc, "ends": 8 * me, "arrive": 4 * nc, "hops": 4 * nc,
                "stage": 4 * nc, "stage_idx": 4 * nc, "cnt": 4 * 65, "rows": 64 * mi, "count": 8}
        check_layout(r, need, per_slot=("mask", "rows", "hops", "count"))
        slots = r["slots"]
        assert r["total_bytes"] <= 4 * gk + 8 * me + (12 + 16 * W + (4 + 8 * W) * slots) * nc + 64 * mi * slots + 256 * (9 + 4 * slots)


def test_plan_at_config_3_and_at_the_key_limit(plan):
    c3, = plan([(1_250_000, 15_000, 15_000, 2, 256, 8)])
    assert (c3["gk"], c3["nc"], c3["words"]) == (30_000, 30_000, 4)
    assert (c3["node_wgs"], c3["edge_wgs"], c3["finish_wgs"], c3["launches"]) == (118, 1024, 1, 20)
    assert c3["total_bytes"] == C3_BYTES
    lim, = plan([(4_000_000, 1 << 20, 1 << 20, 2, 1024, 64)])
    assert (lim["gk"], lim["nc"], lim["words"], lim["node_wgs"], lim["launches"]) == (1 << 21, 1 << 21, 16, 1024, 132)
    assert lim["total_bytes"] == LIMIT_BYTES


# plan_group_impact's totals, worked out by hand from its pieces (each rounded up to 256 bytes):
#   config 3: pos 120 064 + fresh / next 2 x 960 000 + ends 10 000 128 + arrive, stage, stage_idx 3 x 120 064 + cnt 512
#             + 2 slots x (mask 960 000 + rows 16 384 + hops 120 064 + count 256)
#   the limit: pos 8 Mi + fresh / next 2 x 256 Mi + ends 32 000 000 + 3 x 8 Mi + cnt 512 + 2 x (256 Mi + 65 536 + 8 Mi + 256)
C3_BYTES = 120_064 + 2 * 960_000 + 10_000_128 + 3 * 120_064 + 512 + 2 * (960_000 + 16_384 + 120_064 + 256)
LIMIT_BYTES = (8 << 20) + 2 * (256 << 20) + 32_000_000 + 3 * (8 << 20) + 512 + 2 * ((256 << 20) + 65_536 + (8 << 20) + 256)


def test_plan_parameter_checks(plan):
    ok = plan([(1000, 100, 10, 1, mi, mh) for mi, mh in ((1, 1), (1024, 64), (256, 8))])
    assert [r["rc"] for r in ok] == [0] * 3
    bad = plan([(1000, 100, 10, 1, mi, mh) for mi, mh in ((0, 0), (0, 8), (8, 0), (1025, 8), (8, 65), (1 << 32, 8), (8, 1 << 32))])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 7
    assert ok[0]["limit_incidents"] == 1024 and ok[0]["limit_hops"] == 64


def test_header_constants_match_engine(tmp_path):
    names = dict(SG_IMPACT_WORDS=engine.IMPACT_WORDS, SG_IMPACT_MAX_INCIDENTS=engine.IMPACT_MAX_INCIDENTS, SG_IMPACT_MAX_HOPS=engine.IMPACT_MAX_HOPS,
                 SG_NO_HOPS=engine.NO_HOPS, **{"SG_IMPACT_" + f.upper(): i for i, f in enumerate(engine.IMPACT_FIELDS)})
    assert len(engine.IMPACT_FIELDS) == engine.IMPACT_WORDS
    for i, f in enumerate(engine.IMPACT_FIELDS):
        assert getattr(engine, "IMPACT_" + f.upper()) == i
    src = tmp_path / "impact_constants.c"
    src.write_text('#include "servicegraph.h"\n' + "".join(f'_Static_assert((long long)({n}) == {int(v)}LL, "{n} is not {int(v)}");\n' for n, v in names.items()))
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
