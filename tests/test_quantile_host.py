"""The latency percentiles (K20) on the CPU: tests/quantile_ref.py against a second formulation written apart from it (sorted lists of
bin indices, plain Python over the rows), against the oracle's or_percentile_us, and against hand-computed answers for every clause
of Q; the identities between the spaces; and the plan in alaz_amd/csrc/sg_plan.hpp through tests/micro/plan_driver.cpp, stage quantile."""
import ctypes as C
import os

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from oracle import pyoracle
from tests.group_nodes_ref import group_nodes_ref
from tests.group_ref import group_of_ref, group_ref
from tests.helpers import CLOCK
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests import quantile_ref as qr
from tests.traces import _random_map, _random_rows

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP


# ---- a second formulation ------------------------------------------------------------------------------------------------------------
def _expanded_quantile(bins, max_ns, qm):
    """element rank - 1 of the sorted list of bin indices, one entry per request"""
    idx = sorted(b for b, c in enumerate(bins) for _ in range(int(c)))
    if not idx:
        return 0
    total = len(idx)
    rank = max(1, -(-total * qm // 1000))
    b = idx[rank - 1]
    edge = min(int(max_ns) if b == 15 else 2 ** (17 + b), int(max_ns))
    return min(edge // 1000, 2 ** 32 - 1)


def _loop_folds(hist, rows, gmap):
    """{ref: [out bins, in bins]} over the node refs and over the group refs, {(group from, group to): bins}: one row at a time"""
    nodes, work, edges = {}, {}, {}
    g = np.asarray(gmap, dtype=np.uint32).tolist()
    for j in range(len(rows)):
        f, t = int(rows["from_ref"][j]), int(rows["to_ref"][j])
        h = [int(x) for x in hist[j]]
        for table, a, b in ((nodes, f, t), (work, group_of_ref(f, g), group_of_ref(t, g))):
            for ref, side in ((a, 0), (b, 1)):
                e = table.setdefault(ref, [[0] * 16, [0] * 16])
                e[side] = [x + y for x, y in zip(e[side], h)]
        k = (group_of_ref(f, g), group_of_ref(t, g))
        edges[k] = [x + y for x, y in zip(edges.get(k, [0] * 16), h)]
    return nodes, work, edges


def _random_hist(rng, rows):
    """bins that sum to the rows' counts (small ones, so that the expanded lists stay short): alive-only rows are all zero"""
    n = np.minimum(rows["count"], 40).astype(np.int64)
    rows["count"] = n
    h = np.zeros((len(rows), 16), dtype=np.uint32)
    for j in range(len(rows)):
        np.add.at(h[j], rng.integers(0, 16, n[j]), 1)
    return h


@pytest.mark.parametrize("block", range(6))
def test_reference_against_the_second_formulation(block):
    """300 seeds: KNOWN / LABEL / OBIP refs, self-loops, alive-only rows (tests/test_group_host.py's rows), maps that group nothing,
    something and everything"""
    for seed in range(50 * block, 50 * block + 50):
        rng = np.random.default_rng(9000 + seed)
        mk, ml = int(rng.integers(41, 70)), int(rng.integers(1, 8))   # (_random_rows' sources are KNOWN ids below max(mk, ml, 40))
        rows = _random_rows(rng, mk, ml, int(rng.integers(1, 2 * mk)))
        hist = _random_hist(rng, rows)
        mg = int(rng.integers(1, mk + 1))
        gmap = (np.full(mk, NO, np.uint32), _random_map(rng, mk, mg), np.zeros(mk, np.uint32))[seed % 3]
        permille = sorted(set(rng.integers(1, 1001, int(rng.integers(1, 9))).tolist()) | ({500, 990} if seed % 2 else set()))[:8]
        nodes = nodes_ref(rows)
        ge, rg, perm = group_ref(rows, gmap, mg, mk, ml)
        gn = group_nodes_ref(ge, mg, mk, ml)
        assert np.array_equal(qr.row_group(ge, perm), rg)
        HN, HG, HW = qr.fold_nodes(hist, rows, nodes), qr.fold_groups(hist, ge, perm), qr.fold_group_nodes(hist, ge, perm, gn)
        ln, lw, le = _loop_folds(hist, rows, gmap)
        assert [HN[i].tolist() for i in range(len(nodes))] == [ln[int(r)] for r in nodes["ref"]] and len(ln) == len(nodes)
        assert [HW[i].tolist() for i in range(len(gn))] == [lw[int(r)] for r in gn["ref"]] and len(lw) == len(gn)
        assert [HG[i].tolist() for i in range(len(ge))] == [le[(int(a), int(b))] for a, b in zip(ge["from_ref"], ge["to_ref"])] and len(le) == len(ge)
        # the identities: a fold over group edges is a fold over rows; the sum of the bins is the count; nothing grouped: the nodes
        assert HW.tobytes() == qr.fold_group_nodes_over_groups(HG, ge, gn).tobytes()
        assert np.array_equal(HG.sum(axis=1), ge["count"])
        assert np.array_equal(HN[:, 0].sum(axis=1), nodes["out_count"]) and np.array_equal(HW[:, 1].sum(axis=1), gn["in_count"])
        if seed % 3 == 0:
            assert HW.tobytes() == HN.tobytes() and gn["ref"].tobytes() == nodes["ref"].tobytes()
            assert HG.tobytes() == hist.astype(np.uint64).tobytes()
        QN, QG = qr.node_quantiles(HN, nodes, permille), qr.group_quantiles(HG, ge, permille)
        for i in range(len(nodes)):
            for s, mx in ((0, "out_max_ns"), (1, "in_max_ns")):
                assert QN[i, s].tolist() == [_expanded_quantile(HN[i, s], nodes[mx][i], q) for q in permille]
        for i in range(len(ge)):
            assert QG[i].tolist() == [_expanded_quantile(HG[i], ge["max_ns"][i], q) for q in permille]


def test_against_the_oracles_percentile():
    l = pyoracle.lib()
    l.or_percentile_us.restype = C.c_uint32; l.or_percentile_us.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint32]
    rng = np.random.default_rng(5)
    for _ in range(2000):
        h = (rng.integers(0, 1 << int(rng.integers(1, 28)), 16) * (rng.random(16) < 0.4)).astype(np.uint32)
        mx = int(rng.integers(0, 1 << int(rng.integers(1, 45))))
        a = (C.c_uint32 * 16)(*h.tolist())
        for q in (50, 99):
            assert qr.quantile(h, mx, 10 * q) == l.or_percentile_us(a, int(h.sum()), mx, q)


def test_the_sum_of_the_bins_is_the_count_in_the_oracle():
    """every record that adds to a row's count adds to one bin: total = sum of B is count for every row the oracle makes"""
    topo = replay.make_topology(60, 400, seed=3)
    ev, labels = replay.make_events(topo, 20_000, seed=4, mixed=True, with_raw_outbound=True, with_reverse=True)
    o = pyoracle.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    o.packed(ev, labels)
    o.window_close(weights.make_weights(1), 1)
    rows = o.edge_rows()
    h = o.edge_hist()
    assert len(rows) > 100 and len(h) == len(rows) and np.array_equal(h.sum(axis=1), rows["count"])


def test_every_clause_of_q_by_hand():
    z = [0] * 16
    assert qr.quantile(z, 10 ** 9, 990) == 0                                                     # total == 0
    h = list(z); h[3] = 1; h[9] = 1
    assert qr.quantile(h, 1 << 40, 1) == (1 << 20) // 1000                                       # rank ceil(2 / 1000) rounds up to 1: the first request
    assert qr.quantile(h, 1 << 40, 500) == (1 << 20) // 1000 and qr.quantile(h, 1 << 40, 501) == (1 << 26) // 1000
    h = list(z); h[5] = 98; h[9] = 2
    assert [qr.quantile(h, 1 << 40, q) for q in (500, 980, 981, 990, 1000)] == [4194, 4194, 67108, 67108, 67108]
    assert qr.quantile(h, 50_000_000, 990) == 50_000                                             # capped at max_ns
    h = list(z); h[15] = 1
    assert qr.quantile(h, 3_000_000_000, 500) == 3_000_000                                       # the open last bin: max_ns
    assert qr.quantile(h, (1 << 64) - 1, 500) == 0xFFFFFFFF                                      # saturated to u32
    h = list(z); h[0] = 1
    assert qr.quantile(h, 90_000, 500) == 90                                                     # capped inside bin 0
    big = (1 << 55) + 999                                                                        # total * qm would pass 2^64
    h = list(z); h[2] = big; h[4] = big
    total = 2 * big
    assert total * 990 >= 1 << 64
    rank = -(-total * 990 // 1000)
    assert (total // 1000) * 990 + -(-(total % 1000) * 990 // 1000) == rank > big
    assert qr.quantile(h, 1 << 40, 990) == (1 << 21) // 1000 and qr.quantile(h, 1 << 40, 500) == (1 << 19) // 1000
    h[2] = rank; h[4] = total - rank
    assert qr.quantile(h, 1 << 40, 990) == (1 << 19) // 1000                                     # exactly rank requests in front
    h[2] = rank - 1; h[4] = total - rank + 1
    assert qr.quantile(h, 1 << 40, 990) == (1 << 21) // 1000
    q = qr.quantiles(np.array([[h, z], [z, h]], dtype=np.uint64), np.array([[1 << 40, 5], [5, 1 << 40]], dtype=np.uint64), (990,))
    assert q.dtype == np.uint32 and q.tolist() == [[[2097], [0]], [[0], [2097]]]


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("quantile")


def _p(me, ncap, mg, slots=1, spaces=7, world=1, permille=()):
    return (me, ncap, mg, slots, spaces, world, len(permille), *permille)


CASES = [_p(1 << 14, 4500, 4300), _p(1 << 14, 4500, 4300, 3, 5), _p(1_250_000, 30_000, 0, 2), _p(1, 1, 1, 1, 2), _p(0, 0, 0, 0, 7),
         _p(1 << 31, 1 << 20, 1 << 20, 2), _p(4_000_000, 1 << 20, 1 << 20, 2, 4), _p(100, 7, 3, 8, 1, 1, (1, 1000))]


def test_plan_layout_sizes_and_grids(plan):
    for c, r in zip(CASES, plan(CASES)):
        me, ncap, slots, spaces = max(c[0], 1), max(c[1], 1), max(c[3], 1), c[4]
        assert r["rc"] == 0 and r["permille"] == (list(c[7:]) or [500, 990]) and r["lds_bytes"] == 65536 and r["range"] == 512
        caps = (ncap, me, max(r["nc"], 1))
        tot = 0
        for k, s in enumerate(r["space"]):
            assert s["on"] == (spaces >> k) & 1
            if not s["on"]:
                continue
            sides = 1 if k == 1 else 2
            assert s["cap"] == caps[k] and s["sides"] == sides
            ranges = -(-caps[k] // 512)
            assert s["sorted"][0] == ranges and 1 <= s["sorted"][1] <= min(64, -(-me // 2048)) and ranges * s["sorted"][1] * 65536 <= max(256 << 20, ranges * 65536)
            if sides == 2:
                assert s["scattered"][0] == ranges and 1 <= s["scattered"][1] <= min(64, -(-me // 8192))
                assert ranges * s["scattered"][1] * 65536 <= max(256 << 20, ranges * 65536)
            need = dict(part=ranges * max(s["sorted"][1], s["scattered"][1]) * 65536, stage=1024 * sides * 128, stage_idx=4096,
                        tgt_out=4 * me, hist=caps[k] * sides * 128, quantiles=caps[k] * sides * 32)
            if sides == 2:
                need.update(tgt_in=4 * me, pos=4 * (ncap if k == 0 else max(r["gk"], 1)))
            check_layout(dict(s, slots=slots), need, per_slot=("hist", "quantiles"))
            assert 1 <= s["finish_wgs"] <= 1024 and 1 <= s["pos_wgs"] <= 1024 and 1 <= s["tgt_wgs"] <= 1024
            tot += s["total_bytes"]
        assert r["total_bytes"] == tot
        assert r["group_slot_bytes"] == ((r["space"][1]["hist_bytes"] + r["space"][1]["quant_bytes"]) if spaces & 2 else 0)


def test_plan_sizes_are_64_bit_and_config_3(plan, capsys):
    big, c3 = plan([_p(1 << 31, 1 << 20, 1 << 20, 2), _p(1_250_000, 30_000, 0, 2)])
    g = big["space"][1]
    assert g["hist_bytes"] == (1 << 31) * 128 and g["quant_bytes"] == (1 << 31) * 32 and big["tgt_bytes"] == (1 << 31) * 4
    assert g["sorted"] == [1 << 22, 1] and g["part_bytes"] == (1 << 22) * 65536 and big["group_slot_bytes"] == (1 << 31) * 160
    assert big["total_bytes"] > 1 << 39
    g = c3["space"][1]
    assert g["sorted"] == [2442, 1] and c3["group_slot_bytes"] == 1_250_000 * 160
    assert c3["space"][0]["scattered"] == [59, 64] and c3["space"][0]["sorted"] == [59, 64] and c3["space"][2]["sorted"] == [59, 64]
    with capsys.disabled():
        print(f"\n[K20 plan, config 3, two slots] nodes {c3['space'][0]['total_bytes'] / 2**20:.1f} MiB, group edges "
              f"{c3['space'][1]['total_bytes'] / 2**20:.1f} MiB ({c3['group_slot_bytes'] / 2**20:.1f} MiB a slot), workloads "
              f"{c3['space'][2]['total_bytes'] / 2**20:.1f} MiB")


def test_plan_refuses_what_the_header_refuses(plan):
    bad = [_p(100, 10, 0, 1, 8), _p(100, 10, 0, 1, 1, 2), _p(100, 10, 0, 1, 1, 1, (0,)), _p(100, 10, 0, 1, 1, 1, (1001,)),
           _p(100, 10, 0, 1, 1, 1, tuple(range(1, 10))), _p(100, (1 << 21) + 1, 0, 1, 1), _p(100, 1 << 21, 1, 1, 4)]
    for r in plan(bad):
        assert r["rc"] == engine.SG_EINVAL and "space" not in r
    ok = plan([_p(100, 1 << 21, 1, 1, 2), _p(100, 1 << 21, 0, 1, 5), _p(100, 10, 0, 1, 0), _p(100, 10, 0, 1, 7, 1, tuple(range(1, 9)))])
    assert [r["rc"] for r in ok] == [0, 0, 0, 0] and ok[3]["n_q"] == 8 and not any(s["on"] for s in ok[2]["space"])
