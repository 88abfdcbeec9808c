"""K16, the workload rows (sg_set_group_nodes / sg_window_group_nodes / sg_set_group_node_trend / sg_window_group_node_trend /
sg_group_node_trend_entries / sg_window_group_nodes_top / sg_window_group_nodes_select and their *_buffer calls): the workload rows,
their trend rows, the whole baseline, its statistics and the selections of every window against the references of
tests/group_nodes_ref.py, run on the device's own window_groups() and outbound_ips() of that window — byte for byte — and, where it
is cheap, through the formulation over the window's rows; at the boundaries of the out side's fold (spans of 8, chunks of 2048) and
of the in side's ranges (2048 keys) and slices; on every close path; across a rollout; and an engine with it against a twin
without it."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import EXT, RUNS, _d2h, _engine, _events, _feed, _grouped, _hip, _map, _pairs, _pods_engine, _rc, _send
from tests.group_nodes_ref import GroupNodeTrendRef, gk_of_refs, group_nodes_ref, group_nodes_rows, ref_select_group_nodes
from tests.group_ref import group_ref
from tests.helpers import CLOCK, G, HostShim
from tests.node_trend_ref import NodeTrendRef
from tests.nodes_ref import nodes_ref
from tests.traces import churn  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

NO = engine.NO_GROUP
ML = 256                                                              # max_labels of _engine
PARAMS = dict(shift=3, warmup=2, ttl=2)
STATS = ("windows", "entries", "inserted", "expired", "dropped")
INF = float("inf")


def _check(g, mg, mk, ml, rows=None, gmap=None):
    """the last read window's workload rows against the reference over the device's own group edges (and, with rows, over them)"""
    ge = g.window_groups()
    want = group_nodes_ref(ge, mg, mk, ml)
    got = g.window_group_nodes()
    assert len(got) == len(want)
    for f in got.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    assert got.tobytes() == want.tobytes()
    if rows is not None:
        assert got.tobytes() == group_nodes_rows(rows, gmap, mg, mk, ml).tobytes()
    return ge, got


def _check_trend(g, ref, nodes):
    want = ref.window(nodes, g.outbound_ips())
    got = g.window_group_node_trend()
    assert len(got) == len(nodes) and got.tobytes() == want.tobytes()
    assert g.group_node_trend_entries().tobytes() == ref.entries.tobytes()
    s = g.group_node_trend_stats()
    assert tuple(getattr(s, k) for k in STATS) == tuple(ref.stats[k] for k in STATS)
    return want


def _nc(g, mg, mk, ml, mob, max_edges):
    return min(mg + mk + ml + mob, 2 * max_edges)


# ---- 1. the churn -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
def test_churn_is_exact_and_a_twin_without_it_is_unchanged(churn, kind):
    """every window under each map; "one": a single workload holds every out edge of the pods — one long run, the LDS atomics on
    one slot; "none" with the node rollup on: the rows are K9's"""
    topo, labels, wins = churn
    (g, gmap, mk), (twin, _, _) = _grouped(topo, labels, kind), _grouped(topo, labels, kind)
    for x in (g, twin):
        x.set_nodes(); x.set_group_trend(shift=3, warmup=2, ttl=3)
    g.set_group_nodes()
    for i, w in enumerate(wins):
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        ge, n = _check(g, mk, mk, ML, *((rows, gmap) if i in (0, 5) else ()))
        assert ge.tobytes() == twin.window_groups().tobytes()
        assert g.window_row_group().tobytes() == twin.window_row_group().tobytes()
        assert g.window_group_trend().tobytes() == twin.window_group_trend().tobytes()
        assert g.window_nodes().tobytes() == twin.window_nodes().tobytes()
        if kind == "none":
            assert n.tobytes() == g.window_nodes().tobytes()
        else:
            assert n["ref"][0] == G(0) and len(n) < len(g.window_nodes())
            assert n["out_edges"][0] == int((ge["from_ref"] == G(0)).sum())
    assert g.group_trend_entries().tobytes() == twin.group_trend_entries().tobytes()


# ---- constructed windows ---------------------------------------------------------------------------------------------------------

# ---- 2. the out side ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """4200 pods: workload 5 = pods 0, 1 is the caller of the long run; workloads 0..2 = pods 2, 3, 4 come before it in key order;
    everything else is ungrouped"""
    topo, g, mk = _pods_engine(n_pods=4200)
    g.set_groups(); g.group_assign([0, 1, 2, 3, 4], [5, 5, 0, 1, 2])
    g.set_group_nodes()
    gmap = np.full(mk, NO, np.uint32); gmap[:5] = [5, 5, 0, 1, 2]
    return topo, g, mk, gmap


# RUNS (tests/test_gpu_nodes.py, K9's out side over the same list) = (group edges in front of the long run, its length): a run
# inside a span, cut by spans, ending on a chunk end, crossing one, beginning at one, and passing THROUGH a whole chunk


@pytest.mark.parametrize("front,D", RUNS)
def test_out_side_runs_at_the_span_and_chunk_boundaries(wide, front, D):
    topo, g, mk, gmap = wide
    a = front - 3                                                     # workload 0 calls a pods, workload 1 one, workload 2 two
    src = np.concatenate([np.full(a, 2), [3], [4, 4], np.arange(D) % 2, [50, 50, 51]])
    dst = np.concatenate([np.arange(a) + 60, [60], [60, 61], np.arange(D) + 100, [7, 8, 7]])
    rows = _send(topo, g, src, dst)
    ge, n = _check(g, mk, mk, 16, rows, gmap)
    assert len(ge) == front + D + 3 and ge["from_ref"][front] == G(5) == ge["from_ref"][front + D - 1] and ge["from_ref"][front - 1] == G(2)
    w = n[n["ref"] == G(5)][0]
    assert w["out_edges"] == D and w["out_count"] == D and w["in_edges"] == 0
    assert n["ref"][0] == G(0) and n["out_edges"][0] == a


def test_windows_of_no_and_of_one_group_edge(wide):
    topo, g, mk, gmap = wide
    none = np.zeros(0, np.int64)
    rows = _send(topo, g, none, none)
    ge, n = _check(g, mk, mk, 16, rows, gmap)
    assert len(ge) == 0 and len(n) == 0
    rows = _send(topo, g, [0, 1], [1, 0])                             # two rows, one group edge inside workload 5: one node, both sides
    ge, n = _check(g, mk, mk, 16, rows, gmap)
    assert len(ge) == 1 and len(n) == 1 and n["ref"][0] == G(5)
    assert (n["out_edges"][0], n["in_edges"][0], n["out_count"][0], n["in_count"][0]) == (1, 1, 2, 2)
    rows = _send(topo, g, [9], [10])                                  # one row, two ungrouped nodes
    ge, n = _check(g, mk, mk, 16, rows, gmap)
    assert n["ref"].tolist() == [9, 10] and n["out_edges"].tolist() == [1, 0] and n["in_edges"].tolist() == [0, 1]


# ---- 3. the in side ------------------------------------------------------------------------------------------------------------------
MG = 3000                                                             # max_groups + k crosses 4096 at KNOWN id 1096


@pytest.fixture(scope="module")
def ranges():
    """max_edges 65 536: two slices.  GK = 3000 + the node capacity: four ranges of 2048 keys; workloads 2047 and 2048 lie on either
    side of the first range boundary, the KNOWN ids 1095 and 1096 on either side of the second"""
    topo = replay.make_topology(4200, 4 * 4200, seed=7, svcs=4)
    mk = topo.n_nodes + 8
    g = engine.ServiceGraph(max_known_nodes=mk, max_edges=1 << 16, layers=2, max_labels=16, max_outbound_ips=64, max_window_events=1 << 16,
                            max_batch=1 << 14)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(2)
    gmap = np.full(mk, NO, np.uint32)
    gmap[10:20] = 2047; gmap[20:30] = 2048; gmap[30:40] = 7; gmap[40:45] = 2999
    g.set_groups(max_groups=MG); g.group_assign(np.arange(mk), gmap)
    g.set_group_nodes()
    return topo, g, mk, gmap


def test_in_side_ranges_slices_and_every_destination_type(ranges):
    topo, g, mk, gmap = ranges
    rng = np.random.default_rng(3)
    src = rng.integers(0, 4200, 5000)
    dst = np.concatenate([rng.integers(10, 30, 1000), rng.integers(1080, 1110, 1500), rng.integers(0, 4200, 2000), rng.integers(40, 45, 500)])
    pod = _events(topo, src, topo.pod_ips[dst], dur=1_000_000 + 1000 * np.arange(5000, dtype=np.uint64),
                  status=np.where(np.arange(5000) % 7 == 0, 503, 200))
    ext = _events(topo, rng.integers(0, 4200, 300), EXT + rng.integers(0, 2, 300).astype(np.uint32), label=np.repeat([1, 2, 0], 100))
    g.ingest_bulk(np.concatenate([pod, ext]))
    rows = g.flush_window().copy()
    ge, n = _check(g, MG, mk, 16, rows, gmap)
    assert len(ge) > 4096                                             # the slices split the group edges; several chunks on the out side
    t = n["ref"] >> 30
    assert {0, 1, 2, 3} == set(t.tolist()) and (n["in_edges"][t == 1] > 0).all() and (n["in_edges"][t == 2] > 0).all()
    for ref in (G(2047), G(2048), G(2999), 1095, 1096):
        assert n["in_edges"][n["ref"] == ref][0] > 0, ref
    k = gk_of_refs(n["ref"], MG, mk, 16)
    assert {0, 1, 2, 3} <= set((k // 2048).tolist())                   # every range of keys holds a node
    w = n[n["ref"] == G(2047)][0]
    assert w["in_edges"] > 100 and w["in_count"] >= w["in_edges"]


def test_one_callee_receives_from_every_group_edge(ranges):
    topo, g, mk, gmap = ranges
    src = np.concatenate([np.arange(100, 3100), np.arange(10, 40)])   # 3000 ungrouped callers, workloads 2047, 2048 and the callee itself
    rows = _send(topo, g, src, np.concatenate([30 + np.arange(3020) % 10, 30 + (np.arange(10) + 1) % 10]))
    ge, n = _check(g, MG, mk, 16, rows, gmap)
    assert len(ge) == 3003 and (ge["to_ref"] == G(7)).all()
    w = n[n["ref"] == G(7)][0]
    assert (w["in_edges"], w["in_count"], w["out_edges"], w["out_count"]) == (3003, 3030, 1, 10)   # the edge inside it: on both sides
    assert len(n) == 3003


def test_a_window_of_alive_only_rows(ranges):
    topo, g, mk, gmap = ranges
    src, dst = _pairs(150, 2500, 5)
    rows = _send(topo, g, src, dst, alive=np.ones(2500, bool))
    ge, n = _check(g, MG, mk, 16, rows, gmap)
    assert len(n) > 0 and (n["out_count"] == 0).all() and (n["in_count"] == 0).all()
    assert int(n["out_alive"].sum()) == int(n["in_alive"].sum()) == int(rows["alive"].sum()) > 0


# ---- 4. close paths and lifecycle -------------------------------------------------------------------------------------------------------
def test_every_close_path_gives_the_same_rows(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    g.set_group_nodes(); g.set_group_node_trend(**PARAMS)
    ref = GroupNodeTrendRef(_nc(g, mk, mk, ML, 512, 1 << 15), **PARAMS)
    for i, w in enumerate(wins[:7]):
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_group_nodes, g.window_group_node_trend, g.set_group_nodes, g.set_group_node_trend):
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            assert _rc(g.set_group_nodes, False) == engine.SG_ESTATE and _rc(g.window_group_nodes_top, 1) == engine.SG_ESTATE
            g.flush_end()
        elif i == 1:
            g.flush_window_view()
        elif i == 2:
            g.flush_begin(); g.flush_end_view()
        elif i == 3:
            g.flush_window_top(3)
        elif i == 4:
            g.window_run(); g.window_read()
        elif i == 5:
            g.window_close(); g.window_features()
            for l in range(2):
                g.window_layer(l)
            g.window_score(); g.window_read(); g.window_reset()
        else:
            g.flush_window()
        ge, n = _check(g, mk, mk, ML)
        _check_trend(g, ref, n)
    assert g.group_node_trend_stats().windows == 7


def test_window_run_in_flight_under_a_changing_map(churn):
    """sg_window_run with three windows in flight, the map changing between the closes: each window's device buffers, read after the
    round was enqueued, equal the references over a one-call engine's group edges under the same map"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=3), _engine(topo, labels)
    mk = topo.n_nodes + 8
    for x in (g, one):
        x.set_groups(); x.set_group_nodes()
    g.set_group_node_trend(**PARAMS)
    ref = GroupNodeTrendRef(_nc(g, mk, mk, ML, 512, 1 << 15), **PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(wins[:9]):
        lo = 30 * i
        for x in (g, one):
            x.group_assign(np.arange(lo, lo + 40), np.arange(lo, lo + 40) // (3 + i % 4))
        _feed(one, w)
        one.flush_window()
        want = group_nodes_ref(one.window_groups(), mk, mk, ML)
        assert one.window_group_nodes().tobytes() == want.tobytes()
        tr = ref.window(want, one.outbound_ips())
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((want, tr, g.window_group_nodes_buffer(), g.window_group_node_trend_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for want, tr, (np_, cp), tp in pending:
                assert int(_d2h(hip, cp, 1, np.uint64)[0]) == len(want)
                assert _d2h(hip, np_, len(want), engine.NODE_DTYPE).tobytes() == want.tobytes()
                assert _d2h(hip, tp, len(want), engine.NODE_TREND_DTYPE).tobytes() == tr.tobytes()
                sizes.append(len(want))
            pending = []
    assert len(sizes) == 9 and len(set(sizes)) > 3
    assert g.group_node_trend_entries().tobytes() == ref.entries.tobytes()


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    mk = topo.n_nodes + 8
    reads = (g.window_group_nodes, g.window_group_nodes_buffer)
    treads = (g.window_group_node_trend, g.window_group_node_trend_buffer, g.group_node_trend_entries, g.group_node_trend_stats)
    assert _rc(g.set_group_nodes) == engine.SG_ESTATE and _rc(g.set_group_nodes, False) == engine.SG_ESTATE      # the groups are off
    assert _rc(g.set_group_node_trend) == engine.SG_ESTATE and _rc(g.window_group_nodes_top, 1) == engine.SG_ESTATE
    for call in reads + treads:
        assert _rc(call) == engine.SG_ESTATE
    assert g._l.sg_set_group_nodes(g._h, 2) == engine.SG_EINVAL
    g.set_groups(max_groups=1 << 21)                                  # GK = 2^21 + the node capacity
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_nodes()
    assert ei.value.rc == engine.SG_EINVAL and "tighter max_groups" in str(ei.value)
    g.set_groups(); g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7)
    assert _rc(g.set_group_node_trend) == engine.SG_ESTATE             # the workload rows are off
    _feed(g, wins[0]); g.flush_window()
    g.set_group_nodes(); g.set_group_nodes()                          # (again: a no-op)
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE                           # the read window was closed while it was off
    assert _rc(g.window_group_nodes_top, 1) == engine.SG_ESTATE
    for bad in (dict(shift=11), dict(max_entries=(1 << 31) + 1), dict(struct_size=36), dict(reserved=1)):
        assert _rc(g.set_group_node_trend, **bad) == engine.SG_EINVAL
    g.set_group_node_trend(**PARAMS)
    assert _rc(g.window_group_node_trend) == engine.SG_ESTATE and len(g.group_node_trend_entries()) == 0
    _feed(g, wins[1]); g.flush_window()
    ge, n = _check(g, mk, mk, ML)
    ref = GroupNodeTrendRef(_nc(g, mk, mk, ML, 512, 1 << 15), **PARAMS)
    _check_trend(g, ref, n)
    out = np.full(3, 0xFF, np.uint8).repeat(136).view(engine.NODE_DTYPE)      # cap below the count: the count, the first cap rows only
    cnt = C.c_size_t(0)
    assert g._l.sg_window_group_nodes(g._h, out.ctypes.data, 2, C.byref(cnt)) == 0
    assert cnt.value == len(n) > 3 and out[:2].tobytes() == n[:2].tobytes() and out[2:].tobytes() == b"\xff" * 136
    assert g._l.sg_window_group_nodes_top(g._h, 6, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL      # by > SG_NSEL_NEW
    assert g._l.sg_window_group_nodes_top(g._h, 0, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    d_n = C.c_uint64(0)
    assert g._l.sg_window_group_nodes_select(g._h, 6, 1, 0.0, None, None, 0, C.addressof(d_n), None) == engine.SG_EINVAL
    assert g._l.sg_window_group_nodes_select(g._h, 0, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL   # no count word
    g.group_assign([0, 1], [5, NO])                                   # the map does not touch the baseline
    g.set_nodes(); g.set_node_trend(); g.set_nodes(False)             # nor do the node rollup and its baseline
    _feed(g, wins[2]); g.flush_window()
    ge, n = _check(g, mk, mk, ML)
    _check_trend(g, ref, n)
    g.set_group_node_trend(**PARAMS)                                  # re-enabling starts empty
    assert len(g.group_node_trend_entries()) == 0 and g.group_node_trend_stats().windows == 0
    assert _rc(g.window_group_node_trend) == engine.SG_ESTATE and len(g.window_group_nodes_top(2)[0]) == 2
    assert _rc(g.window_group_nodes_top, 2, by="in_lat_dev") == engine.SG_ESTATE
    g.set_group_nodes(False)                                          # takes the baseline with it
    for call in reads + treads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_group_nodes(); g.set_group_node_trend(**PARAMS)
    _feed(g, wins[3]); g.flush_window()
    _check(g, mk, mk, ML)
    g.set_groups()                                                    # any sg_set_groups call frees the stage and what is behind it
    for call in reads + treads:
        assert _rc(call) == engine.SG_ESTATE
    _feed(g, wins[4]); g.flush_window()
    assert _rc(g.window_group_nodes) == engine.SG_ESTATE and len(g.window_groups()) > 0
    g.set_group_nodes()
    g.set_groups(None)
    assert _rc(g.window_group_nodes) == engine.SG_ESTATE and _rc(g.set_group_nodes) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_groups) == engine.SG_EINVAL                       # no groups on a sharded engine, so no workload rows
    assert _rc(g.set_group_nodes) == engine.SG_ESTATE and _rc(g.window_group_nodes) == engine.SG_ESTATE


# ---- 5. the baseline ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def caps(churn, oracle_lib):
    """max_entries per map kind, chosen on the CPU: the reference without a capacity cut over the oracle's rows of the churn's first
    window, under each map — four fifths of the entries it makes, so the first window already drops new entries"""
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    mk = topo.n_nodes + 8
    o.packed(wins[0], labels)
    o.window_close(weights.make_weights(2), 2)
    rows, ob = o.edge_rows(), o.outbound_ips()
    out = {}
    for kind in ("blocks", "one"):
        ref = GroupNodeTrendRef(1 << 15, **PARAMS)
        gmap = _map(kind, mk, topo.n_pods)
        n = group_nodes_ref(group_ref(rows, gmap, mk, mk, ML)[0], mk, mk, ML)
        assert n.tobytes() == group_nodes_rows(rows, gmap, mk, mk, ML).tobytes()
        ref.window(n, ob)
        out[kind] = max(1, len(ref.entries) * 4 // 5)
    return out


@pytest.mark.parametrize("kind", ["blocks", "one"])
def test_baseline_over_the_churn_with_a_capacity_cut_and_expiry(churn, caps, kind):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, kind)
    g.set_group_nodes()
    cap = caps[kind]
    g.set_group_node_trend(max_entries=cap, **PARAMS)
    ref = GroupNodeTrendRef(_nc(g, mk, mk, ML, 512, 1 << 15), max_entries=cap, **PARAMS)
    seen = 0
    for w in wins[:9]:
        _feed(g, w); g.flush_window()
        ge, n = _check(g, mk, mk, ML)
        t = _check_trend(g, ref, n)
        seen += int((t["in_lat_dev"] != 0).sum() + (t["out_err_dev"] != 0).sum())
    assert ref.stats["dropped"] > 0 and ref.stats["expired"] > 0 and seen > 0


def test_default_capacity_is_four_times_the_row_capacity(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    g.set_group_nodes(); g.set_group_node_trend(shift=2, warmup=1)
    ref = GroupNodeTrendRef(_nc(g, mk, mk, ML, 512, 1 << 15), shift=2, warmup=1)
    assert ref.cap == 4 * (2 * mk + ML + 512)
    for w in wins[:3]:
        _feed(g, w); g.flush_window()
        _check_trend(g, ref, _check(g, mk, mk, ML)[1])
    assert ref.stats["dropped"] == 0


def test_a_rollout_keeps_the_workloads_entry_while_the_pods_are_new():
    """workload 0 = pods 0..7 calls workload 1 = pods 20..22: from pods 0..3 for warmup + 2 windows, then from pods 4..7 with the
    latency stepped up.  K10 on the same engine reports the new pods with out_seen == 0; the workload's out side goes on counting"""
    topo, g, mk = _pods_engine()
    warmup = 2
    g.set_groups(); g.group_assign(np.arange(8), 0); g.group_assign(np.arange(20, 23), 1)
    g.set_nodes(); g.set_node_trend(shift=1, warmup=warmup)
    g.set_group_nodes(); g.set_group_node_trend(shift=1, warmup=warmup)
    ncap = mk + 16 + 64
    ref, pod = GroupNodeTrendRef(min(mk + ncap, 1 << 15), shift=1, warmup=warmup), NodeTrendRef(ncap, shift=1, warmup=warmup)
    old, new = np.repeat(np.arange(0, 4), 3), np.repeat(np.arange(4, 8), 3)
    dst = np.tile(np.arange(20, 23), 4)
    other_s, other_d = _pairs(40, 60, 3)                              # steady traffic among ungrouped pods 30..69
    for w in range(warmup + 2):
        _send(topo, g, np.concatenate([old, other_s + 30]), np.concatenate([dst, other_d + 30]))
        _check_trend(g, ref, _check(g, mk, mk, 16)[1])
        assert g.window_node_trend().tobytes() == pod.window(g.window_nodes(), g.outbound_ips()).tobytes()
    _send(topo, g, np.concatenate([new, other_s + 30]), np.concatenate([dst, other_d + 30]),
          dur=np.concatenate([np.full(12, 5_000_000), np.full(60, 1_000_000)]))
    ge, n = _check(g, mk, mk, 16)
    t = _check_trend(g, ref, n)
    pn, pt = g.window_nodes(), g.window_node_trend()
    assert pt.tobytes() == pod.window(pn, g.outbound_ips()).tobytes()
    mine = (pn["ref"] >= 4) & (pn["ref"] < 8)                         # (a KNOWN ref is its id)
    assert mine.sum() == 4 and (pt["out_seen"][mine] == 0).all() and (pt["out_lat_dev"][mine] == 0).all()
    assert n["ref"][0] == G(0) and n["out_count"][0] == 12 and n["out_edges"][0] == 1
    assert t["out_seen"][0] == warmup + 2 and t["out_base_mean_us"][0] == np.float32(1000.0)
    assert t["out_lat_dev"][0] == np.float32(4_000_000 / 1000)        # x = 5 ms against a mean of 1 ms with no deviation: the floor
    assert t["in_seen"][1] == warmup + 2 and n["ref"][1] == G(1)
    new_rows, _, _ = g.window_group_nodes_top(0, by="new")
    assert len(new_rows) == 0                                         # ... and no workload is new
    assert len(g.window_nodes_top(0, by="new")[0]) == 4


def test_regrouping_through_group_assign_alone():
    topo, g, mk = _pods_engine()
    n_pods = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(n_pods), np.arange(n_pods) // 7)
    p = dict(shift=2, warmup=1, ttl=3)
    g.set_group_nodes(); g.set_group_node_trend(**p)
    ref = GroupNodeTrendRef(min(2 * mk + 80, 1 << 15), **p)
    src, dst = _pairs(n_pods, 3000, 41)
    before = None
    for w in range(7):
        if w == 3:
            ids = np.arange(77, n_pods)
            g.group_assign(ids, 30 + ids // 5)                        # pods 77.. (workloads 11..21) move to workloads 45..59
            before = dict(ref.stats)
        _send(topo, g, src, dst, dur=1_000_000 + 50_000 * w)
        ge, n = _check(g, mk, mk, 16)
        t = _check_trend(g, ref, n)
        if w == 3:
            moved = n["ref"] >= G(45)
            assert moved.any() and (t["in_seen"][moved] == 0).all() and (t["in_seen"][~moved] == 3).all()
    assert ref.stats["expired"] - before["expired"] == 2 * 11         # the old workloads' two sides each


def test_index_reads():
    topo, g, mk = _pods_engine()
    n_pods = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(40), np.arange(40) // 2)  # 20 workloads and 110 ungrouped pods
    g.set_group_nodes(); g.set_group_node_trend(shift=1, warmup=1)
    ref = GroupNodeTrendRef(min(2 * mk + 80, 1 << 15), shift=1, warmup=1)
    src, dst = _pairs(n_pods, 6000, 12)
    for w in range(2):
        _send(topo, g, src, dst, dur=1_000_000 * (w + 1))
        ge, n = _check(g, mk, mk, 16)
        t = _check_trend(g, ref, n)
    N = len(n)
    assert N == 130
    assert len(g.window_group_node_trend(np.zeros(0, np.uint32))) == 0
    rep = np.array([5, 5, 0, N - 1, 5], np.uint32)
    assert g.window_group_node_trend(rep).tobytes() == t[rep].tobytes()
    assert _rc(g.window_group_node_trend, np.array([0, N], np.uint32)) == engine.SG_EINVAL
    long = np.random.default_rng(1).integers(0, N, 1025).astype(np.uint32)   # one element longer than the staging's first size
    assert g.window_group_node_trend(long).tobytes() == t[long].tobytes()
    out = np.full(5, 0xFF, np.uint8).repeat(32).view(engine.NODE_TREND_DTYPE)   # cap below the count: the first cap rows only
    cnt = C.c_size_t(0)
    assert g._l.sg_window_group_node_trend(g._h, rep.ctypes.data, 5, out.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == 5 and out[:3].tobytes() == t[rep[:3]].tobytes() and out[3:].tobytes() == b"\xff" * 64


# ---- 6. selection ---------------------------------------------------------------------------------------------------------------------
def _select_all(g, n, tr, torch, bys):
    hip = _hip()
    cap = len(n) + 9
    d_out = torch.zeros(cap * engine.NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    for by in bys:
        v = n["score"] if by == "score" else tr["in_lat_dev" if by == "new" else by]
        mid = float(np.sort(v[np.isfinite(v)])[len(v) // 2])
        for k in (0, 1, 10, len(n) + 5):
            for thr in (-INF, mid, INF):
                want = ref_select_group_nodes(n, tr, by, k, thr)
                rows, idx, n_nodes = g.window_group_nodes_top(k, thr, by=by)
                assert n_nodes == len(n) and idx.tolist() == want.tolist(), (by, k, thr)
                assert rows.tobytes() == n[want].tobytes()
                if by != "score" and len(idx):
                    assert g.window_group_node_trend(idx).tobytes() == tr[idx].tobytes()
                g.window_group_nodes_select(k, thr, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0, by=by)
                torch.cuda.synchronize()
                assert int(d_n.cpu()[0]) == len(want), (by, k, thr)
                assert d_idx.cpu().numpy()[:len(want)].astype(np.uint32).tolist() == want.tolist()
                assert d_out.cpu().numpy()[: len(want) * 136].tobytes() == n[want].tobytes()
    return d_out, d_idx, d_n, cap


def test_selection_host_and_device_forms():
    import torch
    topo, g, mk = _pods_engine()
    gmap = np.full(mk, NO, np.uint32)
    gmap[:90] = np.arange(90) // 6                                    # workloads 0..14; pods 90..149 ungrouped
    g.set_groups(); g.group_assign(np.arange(mk), gmap)
    g.set_group_nodes(); g.set_group_node_trend(shift=2, warmup=1)
    ref = GroupNodeTrendRef(min(2 * mk + 80, 1 << 15), shift=2, warmup=1)
    src, dst = _pairs(90, 1500, 9)
    iso_s, iso_d = np.arange(100, 140, 2), np.arange(101, 141, 2)     # twenty identical isolated pairs: equal scores, ties
    rng = np.random.default_rng(5)
    for w in range(3):
        keep = rng.random(len(src)) < 0.8
        dur = np.concatenate([(1_000_000 * (1 + w * rng.random(int(keep.sum())))).astype(np.uint64), np.full(20, 2_000_000, np.uint64)])
        st = np.concatenate([np.where(rng.random(int(keep.sum())) < 0.1 * w, 503, 200), np.full(20, 200)])
        s_, d_ = np.concatenate([src[keep], iso_s]), np.concatenate([dst[keep], iso_d])
        if w == 2:                                                    # pods 90..99 speak for the first time: new nodes
            s_, d_ = np.concatenate([s_, np.arange(90, 100)]), np.concatenate([d_, np.arange(0, 10)])
            dur, st = np.concatenate([dur, np.full(10, 3_000_000, np.uint64)]), np.concatenate([st, np.full(10, 200)])
        _send(topo, g, s_, d_, dur=dur, status=st)
        ge, n = _check(g, mk, mk, 16)
        tr = _check_trend(g, ref, n)
    iso = n[(n["ref"] >= 100) & (n["ref"] < 140)]
    assert len(iso) == 40 and len(set(iso["score"].tobytes()[i * 4:i * 4 + 4] for i in range(40))) == 1   # the ties
    assert (tr["in_lat_dev"] != 0).any() and (tr["out_err_dev"] != 0).any() and ((tr["in_seen"] == 0) & (tr["out_seen"] == 0)).any()
    d_out, d_idx, d_n, cap = _select_all(g, n, tr, torch, tuple(engine.NSEL_BY))
    g.window_group_nodes_select(5, -INF, d_out.data_ptr(), 0, cap, d_n.data_ptr(), 0)      # rows only
    torch.cuda.synchronize()
    want = ref_select_group_nodes(n, None, "score", 5, -INF)
    assert d_out.cpu().numpy()[: 5 * 136].tobytes() == n[want].tobytes()
    rows, idx, _ = g.window_group_nodes_top(0, cap=4)                 # a cap below the selection
    assert len(rows) == len(idx) == 4 and idx.tolist() == [0, 1, 2, 3] and rows.tobytes() == n[:4].tobytes()
    g.set_group_node_trend(None)                                      # the score needs the workload rows only
    _send(topo, g, np.concatenate([src, iso_s]), np.concatenate([dst, iso_d]))
    ge, n = _check(g, mk, mk, 16)
    _select_all(g, n, None, torch, ("score",))
    for by in ("in_lat_dev", "out_err_dev", "new"):
        assert _rc(g.window_group_nodes_top, 1, by=by) == engine.SG_ESTATE
        assert _rc(g.window_group_nodes_select, 1, 0.0, 0, d_idx.data_ptr(), cap, d_n.data_ptr(), by=by) == engine.SG_ESTATE
