"""K14, the groups, on the host: the pure-Python reference tests/group_ref.py against a formulation written apart from it (numpy
lexsort + reduceat, from_nodes as a count of distinct refs), the dtype against the header's layout, and the plan in
alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage group)."""
import ctypes as C
import os

import numpy as np
import pytest

from alaz_amd import engine, weights
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.group_ref import group_ref
from tests.helpers import CLOCK
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.traces import _random_map, _random_rows
from tests.traces import churn  # noqa: F401  (the fixture: events only, no engine)

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP


def _okey(bits):
    """total order of float32 bit patterns, -0.0 below +0.0 (written apart from group_ref)"""
    b = bits.astype(np.int64)
    return np.where(b < (1 << 31), b + (1 << 31), (1 << 32) - 1 - b)


def group_np(rows, gmap, max_groups, mk, ml):
    """the contract again, on arrays: the keys by np.where, the order by lexsort, the runs by reduceat"""
    E = len(rows)
    gmap = np.asarray(gmap, dtype=np.uint32)

    def keys(ref):
        t, v = (ref >> np.uint32(30)).astype(np.int64), (ref & np.uint32(0x3FFFFFFF)).astype(np.int64)
        g = np.where((t == 0) & (v < len(gmap)), gmap[np.minimum(v, len(gmap) - 1)], NO).astype(np.int64)
        node = np.where(t == 0, v, np.where(t == 1, mk + v, mk + ml + v))
        grouped = g != NO
        return np.where(grouped, g, max_groups + node), np.where(grouped, (3 << 30) | g, ref.astype(np.int64)).astype(np.uint32)

    if E == 0:
        return np.zeros(0, engine.GROUP_EDGE_DTYPE), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    kf, rf = keys(rows["from_ref"]); kt, rt = keys(rows["to_ref"])
    perm = np.lexsort((np.arange(E), kt, kf))
    sf, st = kf[perm], kt[perm]
    starts = np.flatnonzero(np.concatenate(([True], (sf[1:] != sf[:-1]) | (st[1:] != st[:-1]))))
    r = rows[perm]
    out = np.zeros(len(starts), dtype=engine.GROUP_EDGE_DTYPE)
    with np.errstate(over="ignore"):
        for dst, src in (("count", "count"), ("err_count", "err_count"), ("sum_ns", "sum_ns"), ("sumsq_us", "sumsq_us")):
            out[dst] = np.add.reduceat(r[src].astype(np.uint64), starts)
        out["alive"] = np.add.reduceat(r["alive"].astype(np.uint64), starts).astype(np.uint32)
        s = r["score"].astype(np.float32)
        q = np.zeros(E, dtype=np.uint64)
        q[s > 0] = (s[s > 0].astype(np.float64) * 4294967296.0).astype(np.uint64)
        out["score_q32"] = np.add.reduceat(q, starts)
    out["max_ns"] = np.maximum.reduceat(r["max_ns"].astype(np.uint64), starts)
    out["from_ref"], out["to_ref"] = rf[perm][starts], rt[perm][starts]
    out["edges"] = np.diff(np.append(starts, E))
    out["first"] = starts
    run = np.repeat(np.arange(len(starts)), out["edges"])
    ok = _okey(np.ascontiguousarray(s).view(np.uint32))
    best = np.maximum.reduceat(ok, starts)
    cand = np.where(ok == best[run], perm, E)                         # the row indices that hold the run's best score
    out["worst_row"] = np.minimum.reduceat(cand, starts)
    out["score_max"] = rows["score"][out["worst_row"]]
    pairs = np.unique(np.stack([run, r["from_ref"].astype(np.int64)], 1), axis=0)      # distinct (run, from_ref)
    out["from_nodes"] = np.bincount(pairs[:, 0], minlength=len(starts))
    row_group = np.zeros(E, dtype=np.uint32)
    row_group[perm] = run
    return out, row_group, perm.astype(np.uint32)


def _agree(rows, gmap, mg, mk, ml):
    a, b = group_ref(rows, gmap, mg, mk, ml), group_np(rows, gmap, mg, mk, ml)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist()
    return a


@pytest.mark.parametrize("seed", range(10))
def test_reference_against_lexsort_and_reduceat(seed):
    rng = np.random.default_rng(1400 + seed)
    mk, ml = int(rng.integers(4, 200)), int(rng.integers(1, 30))
    rows = _random_rows(rng, mk, ml, int(rng.integers(1, 6 * mk)))
    mg = int(rng.integers(1, mk + 1))
    sizes = set()
    for gmap in (_random_map(rng, mk, mg), _random_map(rng, mk, mg, 1.0, block=7), np.zeros(mk, np.uint32)):
        ge, rg, perm = _agree(rows, gmap, mg, mk, ml)
        assert int(ge["edges"].sum()) == len(rows) and sorted(perm.tolist()) == list(range(len(rows)))
        assert (ge["from_nodes"] >= 1).all() and (ge["from_nodes"] <= ge["edges"]).all()
        sizes.add(int(ge["edges"].max()))
    assert max(sizes) > 1


def test_an_all_ungrouped_map_gives_the_rows_one_to_one():
    rng = np.random.default_rng(7)
    rows = _random_rows(rng, 50, 8, 400)
    ge, rg, perm = _agree(rows, np.full(50, NO, np.uint32), 50, 50, 8)
    E = len(rows)
    assert perm.tolist() == list(range(E)) == rg.tolist() == ge["first"].tolist() == ge["worst_row"].tolist()
    assert (ge["edges"] == 1).all() and (ge["from_nodes"] == 1).all()
    for f in ("count", "err_count", "sum_ns", "sumsq_us", "max_ns", "from_ref", "to_ref", "alive"):
        assert ge[f].tolist() == rows[f].tolist()
    assert ge["score_max"].tobytes() == rows["score"].tobytes()


def test_ties_a_self_edge_and_alive_only_rows():
    K = lambda v: v                                                   # noqa: E731  (a KNOWN ref is its id)
    L = (1 << 30) | 2
    edges = [(K(0), K(5), 0.5), (K(0), K(6), 0.75), (K(1), K(5), 0.75), (K(1), K(1), 0.25), (K(2), K(0), 0.75), (K(2), L, -0.0),
             (K(3), L, 0.0), (K(4), K(9), 0.1)]
    rows = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, (f, t, s) in enumerate(edges):
        rows[i]["from_ref"], rows[i]["to_ref"], rows[i]["score"] = f, t, s
        rows[i]["count"], rows[i]["err_count"], rows[i]["sum_ns"], rows[i]["max_ns"], rows[i]["alive"] = 10 + i, i, 1000 * (i + 1), 100 - i, i % 2
    rows[7]["count"] = rows[7]["err_count"] = rows[7]["sum_ns"] = rows[7]["max_ns"] = 0; rows[7]["alive"] = 3     # alive-only
    gmap = np.full(10, NO, np.uint32)
    gmap[[0, 1, 2]] = 4; gmap[[5, 6]] = 1; gmap[3] = 0               # pods 0-2: workload 4; 5, 6: workload 1; 3: workload 0; 4, 9: none
    ge, rg, perm = _agree(rows, gmap, 8, 10, 4)
    G = lambda g: (3 << 30) | g                                       # noqa: E731
    assert list(zip(ge["from_ref"].tolist(), ge["to_ref"].tolist())) == [(G(0), L), (G(4), G(1)), (G(4), G(4)), (G(4), L), (4, 9)]
    assert perm.tolist() == [6, 0, 1, 2, 3, 4, 5, 7] and rg.tolist() == [1, 1, 1, 2, 2, 3, 0, 4]
    e41 = ge[1]                                                       # three rows, two of them with the best score: the smaller row wins
    assert (e41["edges"], e41["from_nodes"], e41["first"], e41["worst_row"], e41["score_max"], e41["count"]) == (3, 2, 1, 1, 0.75, 33)
    e44 = ge[2]                                                       # traffic inside the workload, the self row among it
    assert (e44["edges"], e44["from_nodes"], e44["worst_row"], e44["max_ns"]) == (2, 2, 4, 97)
    assert np.signbit(ge[3]["score_max"]) and not np.signbit(ge[0]["score_max"])
    quiet = ge[4]
    assert (quiet["count"], quiet["alive"], quiet["edges"], quiet["worst_row"]) == (0, 3, 1, 7)


@pytest.fixture(scope="module")
def oracle_windows(churn, oracle_lib):  # noqa: F811
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    W = weights.make_weights(2)
    out = []
    for w in wins[:6]:
        o.packed(w, labels); o.window_close(W, 2)
        out.append(o.edge_rows())
    return topo, out


def test_oracle_windows_under_random_maps(oracle_windows):
    topo, wins = oracle_windows
    rng = np.random.default_rng(1450)
    mk = topo.n_nodes + 8
    shrink = set()
    for i, rows in enumerate(wins):
        mg = (1, 17, mk)[i % 3]
        gmap = _random_map(rng, mk, mg, share=(1.0, 0.6)[i % 2], block=(None, 7)[i % 2])
        ge, _, _ = _agree(rows, gmap, mg, mk, 256)
        assert (ge["edges"] == np.bincount(_agree(rows, gmap, mg, mk, 256)[1], minlength=len(ge))).all()
        shrink.add(len(ge) < len(rows) // 2)
    assert True in shrink


def test_dtype_and_struct_sizes():
    d = engine.GROUP_EDGE_DTYPE
    assert d.itemsize == 80
    assert [d.fields[f][1] for f in ("count", "score_q32", "from_ref", "to_ref", "edges", "from_nodes", "first", "alive", "worst_row", "score_max")] == \
        [0, 40, 48, 52, 56, 60, 64, 68, 72, 76]
    assert C.sizeof(engine.SgGroupParams) == 16 and NO == 0xFFFFFFFF and engine.REF_GROUP == 3
    hdr = open(os.path.join(HERE, "..", "include", "servicegraph.h")).read()
    assert "#define SG_REF_GROUP 3u" in hdr and "#define SG_NO_GROUP  0xFFFFFFFFu" in hdr and "#define SG_ABI_VERSION 6u" in hdr


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
group_plan = plan_fixture("group")


def _p(me, mk, nc, mg=0, slots=1, world=1, ss=16, r0=0, r1=0):
    return (me, mk, nc, mg, slots, world, ss, r0, r1)


def test_plan_passes_and_key_width(group_plan):
    """2 kb = 16, 18, 30, 32 and 34: two-, three-, four- and five-pass plans, u32 keys up to 32 bits and u64 beyond; at both ends of
    each width"""
    for kb, passes, kbytes in ((8, 2, 4), (9, 3, 4), (15, 4, 4), (16, 4, 4), (17, 5, 8)):
        for gk in ((1 << (kb - 1)) + 1, 1 << kb):
            nc = 100
            r, = group_plan([_p(1 << 15, 64, nc, gk - nc)])
            assert r["rc"] == 0 and (r["gk"], r["kb"], r["passes"], r["key_bytes"]) == (gk, kb, passes, kbytes), (kb, gk, r)
            assert r["keys_bytes"] >= (1 << 15) * kbytes
    c3, = group_plan([_p(1_250_000, 10_000, 15_000)])                  # config 3: max_groups = max_known, 15 + 15 bits
    assert (c3["max_groups"], c3["kb"], c3["passes"], c3["key_bytes"]) == (10_000, 15, 4, 4)
    wide, = group_plan([_p(1 << 20, 1 << 20, (1 << 20) + 5000, 1 << 30)])
    assert (wide["kb"], wide["passes"], wide["key_bytes"]) == (31, 8, 8)


def test_plan_sizes(group_plan):
    for r in group_plan([_p(me, mk, mk + 300, 0, slots) for me, mk in ((1, 1), (4096, 800), (4097, 800), (1 << 15, 6308), (1_250_000, 10_000), (1 << 23, 1 << 20))
                         for slots in (1, 3, 8)]):
        assert r["rc"] == 0 and r["edge_size"] == 80 and r["params_size"] == 16 and r["max_groups"] == r["max_known"]
        me, slots = r["max_edges"], r["slots"]
        assert (r["tile"], r["chunk"], r["max_wgs"]) == (4096, 2048, 1024)
        assert r["tiles"] * 4096 >= me > (r["tiles"] - 1) * 4096 and r["chunks"] * 2048 >= me > (r["chunks"] - 1) * 2048
        assert r["key_wgs"] * 1024 >= me and 1 <= r["heads_wgs"] <= 1024 and r["heads_wgs"] * r["cpw"] >= r["chunks"] > (r["heads_wgs"] - 1) * r["cpw"]
        assert r["stitch_wgs"] * 256 >= r["chunks"]
        assert r["idx_bytes"] >= 4 * me and r["map_bytes"] >= 4 * r["max_known"] and r["hist_bytes"] >= 1024 * r["tiles"]
        assert r["chunkcnt_bytes"] >= 4 * r["chunks"] and r["part_bytes"] >= 160 * r["chunks"] and r["meta_bytes"] >= 8 * r["chunks"]
        assert r["blk_bytes"] >= 2 * 1024 * 4 and r["rows_bytes"] >= 80 * me and r["count_bytes"] >= 8
        names = ("keys_bytes", "idx_bytes", "map_bytes", "hist_bytes", "chunkcnt_bytes", "part_bytes", "meta_bytes", "blk_bytes", "stage_bytes",
                 "rows_bytes", "count_bytes")
        assert all(r[k] % 256 == 0 for k in names)
        assert r["total_bytes"] == (2 * r["keys_bytes"] + 2 * r["idx_bytes"] + r["map_bytes"] + r["hist_bytes"] + r["chunkcnt_bytes"] + r["part_bytes"]
                                    + r["meta_bytes"] + r["blk_bytes"] + 2 * r["stage_bytes"]
                                    + slots * (r["rows_bytes"] + 2 * r["idx_bytes"] + r["count_bytes"]))
        check_layout(r, {"keys0": me * r["key_bytes"], "keys1": me * r["key_bytes"], **{k: 4 * me for k in ("idx0", "idx1", "row_group", "perm")},
                         "map": 4 * r["max_known"], "hist": 1024 * r["tiles"], "chunkcnt": 4 * r["chunks"], "part": 160 * r["chunks"],
                         "meta": 8 * r["chunks"], "blk": 2 * 1024 * 4, "stage": 4 * 65536, "stage_idx": 4 * 65536, "rows": 80 * me, "count": 8},
                     per_slot=("rows", "count", "row_group", "perm"))
    c3, = group_plan([_p(1_250_000, 10_000, 15_000)])
    assert (c3["tiles"], c3["chunks"], c3["cpw"], c3["heads_wgs"]) == (306, 611, 1, 611)
    big, = group_plan([_p(1 << 23, 1 << 20, (1 << 20) + 300)])
    assert (big["chunks"], big["cpw"], big["heads_wgs"]) == (4096, 4, 1024)


def test_plan_parameter_checks(group_plan):
    ok = group_plan([_p(1000, 100, 150), _p(1000, 100, 150, 7), _p(1000, 100, 150, 1 << 30)])
    assert [r["rc"] for r in ok] == [0] * 3 and [r["max_groups"] for r in ok] == [100, 7, 1 << 30]
    bad = group_plan([_p(1000, 100, 150, world=2), _p(1000, 100, 150, ss=12), _p(1000, 100, 150, ss=20), _p(1000, 100, 150, r0=1),
                      _p(1000, 100, 150, r1=1), _p(1000, 100, 150, (1 << 30) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 6


# ---- GraphDS: the owner resolution against the recording stand-in ------------------------------------------------------------------
SET = 0xFFFFFFFE                                                      # the stand-in's mark of an sg_set_groups call


@pytest.fixture()
def ds():
    from alaz_amd import hostlib
    return hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)


def _ops(g):
    return [tuple(int(x) for x in r) for r in g.mock_group_ops()]


def test_graphds_resolves_pods_to_their_top_known_owner(ds):
    assert ds.set_workload_groups(0) == 0 and _ops(ds) == [(SET, 0)]
    ds.PersistReplicaSet("rs-a", "dep-a")                             # the ReplicaSet first: its pods go straight to the Deployment
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")
    ds.PersistPodOwned("pod-1", "10.0.0.2", "rs-b")                   # its ReplicaSet is unknown so far: the ReplicaSet is the group
    ds.PersistPodOwned("pod-2", "10.0.0.3", "ds-x")                   # a DaemonSet owner, as it is
    ds.PersistPodOwned("pod-3", "10.0.0.4", "")                       # no owner: ungrouped, no call
    ds.PersistPodOwned("pod-4", "10.0.0.5", "rs-a")
    assert _ops(ds)[1:] == [(0, 0), (1, 1), (2, 2), (4, 0)]           # group ids in arrival order: dep-a, rs-b, ds-x
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a", "UPDATE")         # nothing changed: no call
    assert len(_ops(ds)) == 5
    ds.PersistReplicaSet("rs-b", "dep-b")                             # after its pod: the pod moves to the Deployment's group
    assert _ops(ds)[5:] == [(1, 3)]
    ds.PersistReplicaSet("rs-b", "dep-b", "UPDATE")
    ds.PersistReplicaSet("rs-c", "")                                  # a ReplicaSet of its own: a pod of it is grouped by the ReplicaSet
    ds.PersistPodOwned("pod-5", "10.0.0.6", "rs-c")
    assert _ops(ds)[6:] == [(5, 4)]


def test_graphds_delete_and_a_late_switch(ds):
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")
    ds.PersistService("svc-0", "10.1.0.1")
    ds.PersistPodOwned("pod-2", "10.0.0.3", "rs-a")
    assert _ops(ds) == []                                             # off: the owners are remembered, nothing is sent
    assert ds.set_workload_groups(8) == 0
    assert _ops(ds) == [(SET, 8), (0, 0), (1, 1), (3, 0)]             # the pods known so far, in id order (id 2 is the service)
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q", "DELETE")
    assert len(_ops(ds)) == 4                                         # the open window may still name it
    ds.FlushWindow(1000)
    assert _ops(ds)[4:] == [(1, engine.NO_GROUP)]                     # its id is released: out of its group
    assert len(ds.workload_edges()) == 0                              # (the stand-in has no rows)
    ds.PersistPodOwned("pod-9", "10.0.0.9", "sts-q")                  # the id comes back for another pod
    assert _ops(ds)[5:] == [(1, 1)]
