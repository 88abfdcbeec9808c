"""K23, the traffic baselines (sg_set_traffic_trend / sg_window_traffic / sg_window_node_traffic / sg_window_group_traffic /
sg_window_group_node_traffic / sg_window_traffic_buffer / sg_traffic_trend_entries / sg_traffic_trend_stats_get and the three
_top_traffic selections): the traffic rows, the whole baseline and its statistics of every space after every window against the
references of tests/traffic_ref.py — byte for byte — run on the same engine's own rows, node rows, group edges, workload rows and
outbound IPs of that window.  Engines are small (max_edges <= 2^15); the shapes are those of tests/test_gpu_node_trend.py,
tests/test_gpu_group_trend.py and tests/test_gpu_quantile_trend.py: K8's walk takes one workgroup per 2048 merged elements.
Every test passes explicit floors; how the defaults resolve is tests/test_traffic_host.py's."""
import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import _d2h, _engine, _feed, _hip, _map, _pairs, _pods_engine, _rc, _send
from tests.helpers import G
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)
from tests.traffic_ref import EdgeTrafficRef, GroupTrafficRef, NodeTrafficRef, WorkloadTrafficRef, ref_select_traffic, traffic_column

pytestmark = pytest.mark.gpu

NO = engine.NO_GROUP
ALL = ("edges", "nodes", "groups", "group_nodes")
STATS = ("windows", "entries", "inserted", "expired", "dropped")
FLOORS = dict(rate_floor=2, load_floor_ns=50_000)
PARAMS = dict(shift=3, warmup=2, ttl=3, max_entries=700, **FLOORS)   # a small ttl, and a capacity the churn overflows
INF = float("inf")

#: per space: the entity rows' read (the edge rows come from the flush), the traffic read
READS = dict(edges=(None, "window_traffic"), nodes=("window_nodes", "window_node_traffic"), groups=("window_groups", "window_group_traffic"),
             group_nodes=("window_group_nodes", "window_group_node_traffic"))


def _stages(g, gmap=None):
    g.set_nodes(); g.set_groups()
    if gmap is not None:
        g.group_assign(np.arange(len(gmap)), gmap)
    g.set_group_nodes()


class Traffic:
    """the references of one engine's traffic baselines and the check of the last read window against them"""

    def __init__(self, g, mk, spaces=ALL, **params):
        ncap = g.window_buffers()[3]
        nc = min(mk + ncap, 2 * g.max_edges)                          # (max_groups defaults to max_known_nodes)
        self.spaces = spaces
        make = dict(edges=lambda: EdgeTrafficRef(g.max_edges, **params), nodes=lambda: NodeTrafficRef(ncap, **params),
                    groups=lambda: GroupTrafficRef(g.max_edges, **params), group_nodes=lambda: WorkloadTrafficRef(nc, **params))
        self.ref = {s: make[s]() for s in spaces}
        g.set_traffic_trend(spaces, **params)

    def check(self, g, rows):
        """rows: the window's edge rows as the flush returned them"""
        out = {}
        for s in self.spaces:
            ents = rows if s == "edges" else getattr(g, READS[s][0])()
            want = self.ref[s].window(ents, g.outbound_ips())
            got = getattr(g, READS[s][1])()
            assert len(got) == len(ents) and got.dtype == want.dtype, s
            for f in got.dtype.names:
                assert got[f].tobytes() == want[f].tobytes(), (s, f)
            ref = self.ref[s]
            assert g.traffic_trend_entries(s).tobytes() == ref.entries.tobytes(), s
            st = g.traffic_trend_stats(s)
            assert tuple(getattr(st, k) for k in STATS) == tuple(ref.stats[k] for k in STATS), s
            out[s] = (ents, got)
        return out


def _twin_reads(g):
    calls = ["window_nodes", "window_groups", "window_group_nodes", "window_group_perm", "window_hist", "window_node_hist",
             "window_node_quantiles", "window_group_hist", "window_group_quantiles", "window_group_node_hist", "window_group_node_quantiles",
             "window_trend", "window_node_trend", "window_group_trend", "window_group_node_trend", "trend_entries", "node_trend_entries",
             "group_trend_entries", "group_node_trend_entries", "window_node_quantile_trend", "window_group_quantile_trend",
             "window_group_node_quantile_trend"]
    out = {c: getattr(g, c)().tobytes() for c in calls}
    for s in ("nodes", "groups", "group_nodes"):
        out["tail entries " + s] = g.quantile_trend_entries(s).tobytes()
    return out


# ---- 1. the churn: exact in four spaces, a twin without the stage unchanged ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "blocks"])
def test_churn_is_exact_and_a_twin_without_the_stage_is_unchanged(churn, kind):
    """entities that come and go, LABEL and OBIP keys (Host labels, raw outbound IPs whose list index changes), alive-only entities,
    ttl 3 and a capacity the churn overflows.  Both engines keep the four mean baselines, K20 and K21 with the same parameters from
    the same window: every other output is the twin's byte for byte.  "none": the workload space is the node space, and the
    group-edge space is the pod-edge space but for the key's type shift."""
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    gmap = _map(kind, mk, topo.n_pods)
    mean = dict(shift=3, warmup=2, ttl=3, max_entries=700)
    g, twin = (_engine(topo, labels, variant=2, edge_histogram=True) for _ in range(2))
    for x in (g, twin):
        _stages(x, gmap)
        x.set_quantiles(("nodes", "groups", "group_nodes"))
        x.set_trend(**mean); x.set_node_trend(**mean); x.set_group_trend(**mean); x.set_group_node_trend(**mean)
        x.set_quantile_trend(("nodes", "groups", "group_nodes"), 990, **mean)
    tr = Traffic(g, mk, **PARAMS)
    moved, types = 0, set()
    for w in wins[:9]:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        a, b = _twin_reads(g), _twin_reads(twin)
        for c in a:
            assert a[c] == b[c], c
        t = tr.check(g, rows)
        if kind == "none":
            assert t["group_nodes"][1].tobytes() == t["nodes"][1].tobytes() and t["groups"][1].tobytes() == t["edges"][1].tobytes()
            wk, nk = g.traffic_trend_entries("group_nodes"), g.traffic_trend_entries("nodes")
            assert np.array_equal(wk["from_key"], nk["from_key"] + np.uint64(1 << 32))    # the key's type shift, nothing else
            for f in ("to_key", "lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last"):
                assert wk[f].tobytes() == nk[f].tobytes(), f
        moved += int((t["nodes"][1]["in_lat_dev"] != 0).sum()) + int((t["edges"][1]["err_dev"] != 0).sum())
        types |= set((g.traffic_trend_entries("edges")["to_key"] >> np.uint64(32)).tolist())
    assert moved > 0 and types >= {0, 1, 2}                           # KNOWN, LABEL and OBIP keys in the baseline
    assert all(tr.ref[s].stats["dropped"] > 0 and tr.ref[s].stats["expired"] > 0 for s in ("edges", "nodes"))


# ---- 2. several workgroups ----------------------------------------------------------------------------------------------------------------
def test_default_capacities_across_workgroups(churn, warm_stream):
    """the default capacities: 4 x ncap + 2 x ncap merged elements of the node space are at least four K8 workgroups, 2 x max_edges +
    max_edges of the two edge-shaped spaces 48: spans cross workgroups (the node-shaped spaces of the 140-pod engines below run
    one workgroup, their edge-shaped spaces 24)"""
    for (topo, labels, wins), n in ((warm_stream, 5), (churn, 4)):
        g = _engine(topo, labels, max_obip=1024, max_window_events=700_000)
        mk = topo.n_nodes + 8
        _stages(g, _map("blocks", mk, topo.n_pods))
        tr = Traffic(g, mk, shift=2, warmup=1, ttl=5, **FLOORS)
        ncap = g.window_buffers()[3]
        assert (6 * ncap + 2047) // 2048 >= 4 and (3 * g.max_edges + 2047) // 2048 == 48
        for w in wins[:n]:
            _feed(g, w)
            t = tr.check(g, g.flush_window().copy())
        assert len(t["groups"][0]) > 256 and (t["groups"][1]["lat_dev"] != 0).any() and (t["edges"][1]["lat_dev"] != 0).any()
        assert tr.ref["groups"].cap == tr.ref["edges"].cap == 2 * g.max_edges and tr.ref["nodes"].cap == 4 * ncap


# ---- 3. k1_variant 0, 1 and 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_k1_variants(churn, variant):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=variant)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    tr = Traffic(g, mk, **PARAMS)
    for w in wins[:5]:
        _feed(g, w)
        t = tr.check(g, g.flush_window().copy())
    assert (t["nodes"][1]["in_base_mean_us"] != 0).any() and (t["edges"][1]["base_mean_us"] != 0).any()


# ---- 4. constructed windows: the boundaries, the sides, a rollout -----------------------------------------------------------------------
@pytest.fixture()
def small():
    topo, g, mk = _pods_engine(n_pods=140)
    gmap = np.full(mk, NO, np.uint32); gmap[:8] = 0                   # workload 0 = pods 0 .. 7
    _stages(g, gmap)
    return topo, g, mk


def test_windows_of_zero_one_and_two_entities_first_expired_and_alive_only(small):
    topo, g, mk = small
    tr = Traffic(g, mk, shift=1, warmup=1, ttl=2, **FLOORS)
    none = np.zeros(0, np.int64)
    t = tr.check(g, _send(topo, g, none, none))                       # the first window: B = 0, E = 0 in every space
    assert all(len(t[s][1]) == 0 and len(g.traffic_trend_entries(s)) == 0 and g.traffic_trend_stats(s).windows == 1 for s in ALL)
    t = tr.check(g, _send(topo, g, [20] * 3, [21] * 3, dur=3_000_000))    # B = 0, one edge of three requests: two node rows
    assert [len(t[s][1]) for s in ALL] == [1, 2, 1, 2]
    assert [len(g.traffic_trend_entries(s)) for s in ALL] == [1, 2, 1, 2]                # a node that only calls, one that is only called
    e = g.traffic_trend_entries("nodes")
    assert list(zip(e["from_key"].tolist(), e["to_key"].tolist())) == [(20, 1), (21, 0)] and e["lat_mean"].tolist() == [3000.0, 3000.0]
    assert e["err_mean"].tolist() == [9_000_000.0, 9_000_000.0]
    t = tr.check(g, _send(topo, g, [20] * 6 + [22], [21] * 6 + [21], dur=3_000_000))     # two edges; the first doubles
    ed = t["edges"][1]
    assert ed["windows_seen"].tolist() == [1, 0] and ed["base_mean_us"].tolist() == [3.0, 0.0]
    assert ed["lat_dev"].tolist() == [1.5, 0.0] and ed["err_dev"][0] == np.float32(9_000_000 / 50_000)   # (6000 - 3000) / (1000 * 2)
    nt = t["nodes"][1][t["nodes"][0]["ref"] == 21][0]
    assert nt["in_seen"] == 1 and nt["in_lat_dev"] == 2.0 and nt["out_seen"] == 0 and nt["out_lat_dev"] == 0   # 7 requests against 3
    t = tr.check(g, _send(topo, g, [20, 22], [21, 21], alive=[True, False]))             # an alive-only row beside a live one
    ed = t["edges"][1]
    assert ed["lat_dev"][0] == 0 and ed["windows_seen"].tolist() == [2, 1] and ed["base_mean_us"][0] == 4.5 and ed["lat_dev"][1] == 0
    assert g.traffic_trend_entries("edges")["n"].tolist() == [2, 2]                      # the alive-only row refreshed nothing
    for _ in range(2):
        tr.check(g, _send(topo, g, none, none))                       # ttl 2: everything expires
    assert all(g.traffic_trend_stats(s).entries == 0 and g.traffic_trend_stats(s).expired > 0 for s in ALL)
    src, dst = _pairs(30, 200, 3)
    t = tr.check(g, _send(topo, g, src + 20, dst + 20))               # a window after everything expired
    assert all((t[s][1][f] == 0).all() for s, f in (("edges", "windows_seen"), ("nodes", "in_seen"), ("groups", "windows_seen"), ("group_nodes", "out_seen")))


@pytest.mark.parametrize("E", [255, 256, 257])
def test_matched_pairs_across_thread_spans_and_workgroups(E):
    """E samples against a baseline that holds the same E keys: 2 E merged elements over the 24 workgroups the default capacity of
    a 2^14-edge engine plans, one element a thread — every matched entry / sample pair straddles two spans, and one of them two
    workgroups.  Then an over-capacity window: more new keys than room."""
    topo, g, mk = _pods_engine(n_pods=140)
    _stages(g, np.full(mk, NO, np.uint32))
    tr = Traffic(g, mk, shift=1, warmup=1, ttl=4, **FLOORS)
    assert (3 * g.max_edges + 2047) // 2048 == 24
    src, dst = _pairs(30, E, 11)
    rep = 1 + np.arange(E) % 3
    for k in (1, 2, 1):                                               # the same keys, the counts doubled and back
        t = tr.check(g, _send(topo, g, np.repeat(src, rep * k) + 20, np.repeat(dst, rep * k) + 20))
        assert len(t["edges"][1]) == len(t["groups"][1]) == E
    assert (t["edges"][1]["windows_seen"] == 2).all() and (t["edges"][1]["lat_dev"] < 0).all() and (t["groups"][1]["err_dev"] < 0).all()
    tight = Traffic(g, mk, spaces=("edges", "groups"), shift=1, warmup=1, ttl=4, max_entries=E - 7, **FLOORS)
    for _ in range(2):                                                # over capacity: seven new keys dropped, twice
        tight.check(g, _send(topo, g, src + 20, dst + 20))
    assert g.traffic_trend_stats("edges").dropped == 14 and g.traffic_trend_stats("groups").entries == E - 7


def test_a_rollout_keeps_the_workload_baseline_and_starts_new_pod_entries(small):
    """every pod of workload 0 replaced (pods 0 .. 3 leave, 4 .. 7 take their traffic): SG_T_NODES starts new entries, SG_T_GROUP_NODES
    keeps the baseline of workload 0 and sees no change of rate"""
    topo, g, mk = small
    tr = Traffic(g, mk, shift=1, warmup=2, **FLOORS)
    old, new, dst = np.repeat(np.arange(0, 4), 3), np.repeat(np.arange(4, 8), 3), np.tile(np.arange(20, 23), 4)
    for w in range(4):
        tr.check(g, _send(topo, g, old, dst, dur=2_000_000))
    t = tr.check(g, _send(topo, g, new, dst, dur=2_000_000))
    gn, wt = t["group_nodes"]
    k = int(np.flatnonzero(gn["ref"] == G(0))[0])
    assert wt["out_seen"][k] == 4 and wt["out_base_mean_us"][k] == 12.0 and wt["out_lat_dev"][k] == 0 and wt["out_err_dev"][k] == 0
    nodes, nt = t["nodes"]
    assert (nt["out_seen"][np.isin(nodes["ref"], np.arange(4, 8))] == 0).all()
    assert len(g.traffic_trend_entries("nodes")) == 8 + 3 and len(g.traffic_trend_entries("group_nodes")) == 1 + 3


# ---- 5. every close path ----------------------------------------------------------------------------------------------------------------
def test_every_close_path(churn):
    """the window's rows for the pod-edge reference come from a twin that closes every window with sg_flush_window (a selecting
    flush returns only the selected rows); where the path returns every row they are the twin's"""
    topo, labels, wins = churn
    g, one = (_engine(topo, labels, variant=2, max_edges=1 << 14) for _ in range(2))
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    g.set_trend(shift=3, warmup=1)                                    # (for the _top_by flush)
    tr = Traffic(g, mk, **PARAMS)
    for i, w in enumerate(wins[:8]):
        _feed(g, w); _feed(one, w)
        rows, got = one.flush_window().copy(), None
        if i == 0:
            g.flush_begin()
            for call in (g.window_node_traffic, g.window_group_traffic, g.window_group_node_traffic, g.set_traffic_trend,
                         g.window_nodes_top_traffic, g.window_groups_top_traffic, g.window_group_nodes_top_traffic):
                assert _rc(call, *((1,) if "top" in call.__name__ else ())) == engine.SG_ESTATE     # a flush is open
            got = g.flush_end()
        elif i == 1:
            got = g.flush_window_view()
        elif i == 2:
            g.flush_begin(); got = g.flush_end_view()
        elif i == 3:
            g.flush_window_top(3)
        elif i == 4:
            g.window_run(); got = g.window_read()
        elif i == 5:
            g.window_close(); g.window_features()
            for l in range(2):
                g.window_layer(l)
            g.window_score(); got = g.window_read(); g.window_reset()
        elif i == 6:
            g.flush_window_top(2, by="lat_dev")                       # sg_flush_window_top_by
        else:
            g.flush_begin(); g.flush_end_top(2)
        assert got is None or np.array(got).tobytes() == rows.tobytes()
        tr.check(g, rows)


# ---- 6. three windows in flight -----------------------------------------------------------------------------------------------------------
def test_window_run_three_in_flight_through_the_device_buffers(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, windows_in_flight=3)
    one = _engine(topo, labels, variant=2, max_edges=1 << 14)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    for x in (g, one):
        _stages(x, gmap)
    tr = Traffic(one, mk, **PARAMS)
    g.set_traffic_trend(ALL, **PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(wins[:6]):
        _feed(one, w)
        t = tr.check(one, one.flush_window().copy())
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((t, [g.window_traffic_buffer(s) for s in ALL]))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for t, bufs in pending:
                for s, p in zip(ALL, bufs):
                    want = t[s][1]
                    assert _d2h(hip, p, want.nbytes, np.uint8).tobytes() == want.tobytes(), s
                sizes.append(len(t["nodes"][0]))
            pending = []
    assert len(sizes) == 6 and len(set(sizes)) > 1
    for s in ALL:                                                     # the state updates ran in window order
        assert g.traffic_trend_entries(s).tobytes() == tr.ref[s].entries.tobytes()


# ---- 7. the selections ----------------------------------------------------------------------------------------------------------------------
def _tops(g):
    return (("nodes", g.window_nodes_top_traffic, ("in", "out")), ("group_nodes", g.window_group_nodes_top_traffic, ("in", "out")),
            ("groups", g.window_groups_top_traffic, (None,)))


def _select_all(g, t, ks, thresholds):
    """every direction and side of every selectable space against ref_select_traffic; thresholds(v): the min_values for column v"""
    for s, top, sides in _tops(g):
        ents, tr = t[s]
        for by in engine.TSEL_BY:
            for side in sides:
                kw = dict(by=by) if side is None else dict(by=by, side=side)
                v = traffic_column(tr, by, side)
                for k in ks(len(ents)):
                    for thr in thresholds(v):
                        want = ref_select_traffic(tr, by, side, k, thr)
                        rows, idx, n = top(k, thr, **kw)
                        assert n == len(ents) and idx.tolist() == want.tolist(), (s, by, side, k, thr)
                        assert rows.tobytes() == ents[want].tobytes()


def test_the_selections_over_the_churn(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    tr = Traffic(g, mk, shift=3, warmup=1, **FLOORS)
    for w in wins[:3]:
        _feed(g, w)
        t = tr.check(g, g.flush_window().copy())
    assert (t["nodes"][1]["in_lat_dev"] > 0).any() and (t["nodes"][1]["in_lat_dev"] < 0).any()
    # k of 0, 1, a few and more than the rows; no threshold, one that cuts (the median of the signed column), one nothing passes
    _select_all(g, t, lambda n: (0, 1, 7, n + 5), lambda v: (-INF, float(np.sort(v)[len(v) // 2]), INF))
    up, down = g.window_nodes_top_traffic(7, by="surge", side="in")[1].tolist(), g.window_nodes_top_traffic(7, by="drop", side="in")[1].tolist()
    assert up != down                                                 # the sign is part of the key
    L = g._l
    for by in (0, 1, 3, 12, 13, 16, 20):                              # a node-shaped space: no side, both sides, an unknown bit
        assert L.sg_window_nodes_top_traffic(g._h, by, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL, by
        assert L.sg_window_group_nodes_top_traffic(g._h, by, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL, by
    for by in (4, 5, 8, 11, 16):                                      # the group edges have no side
        assert L.sg_window_groups_top_traffic(g._h, by, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL, by
    assert L.sg_window_group_nodes_top_traffic(g._h, 5, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    assert L.sg_window_groups_top_traffic(g._h, 1, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL


def test_ties_of_zero_and_a_window_where_everything_falls():
    """a ring of 30 pods, each calling the next two, in blocks of three: every node and workload has both sides.  Window 2 repeats
    window 1: every deviation is +0.0, and -0.0 under a falling key — one key, ties by row position.  Window 3 sends a third of
    the traffic: every deviation is negative, a rising key selects nothing at min_value 0 and a falling one everything"""
    topo, g, mk = _pods_engine(n_pods=140)
    gmap = np.full(mk, NO, np.uint32); gmap[20:50] = np.arange(30) // 3
    _stages(g, gmap)
    tr = Traffic(g, mk, shift=1, warmup=1, **FLOORS)
    ring = np.arange(30)
    src, dst = np.concatenate([ring, ring]) + 20, np.concatenate([(ring + 1) % 30, (ring + 2) % 30]) + 20
    for _ in range(2):
        t = tr.check(g, _send(topo, g, np.repeat(src, 3), np.repeat(dst, 3)))
    for s, cols in (("nodes", ("in_lat_dev", "in_err_dev", "out_lat_dev", "out_err_dev")), ("groups", ("lat_dev", "err_dev"))):
        for c in cols:
            assert (t[s][1][c].view(np.uint32) == 0).all() and (t[s][1][c.replace("lat_dev", "seen").replace("err_dev", "seen") if s == "nodes" else "windows_seen"] == 1).all()
    _select_all(g, t, lambda n: (0, 1, 4, n + 1), lambda v: (-INF, 0.0, -0.0, 1e-30))
    rows, idx, n = g.window_nodes_top_traffic(4, 0.0, by="drop", side="out")
    assert idx.tolist() == [0, 1, 2, 3] and n == 30                   # -0.0 >= 0.0, and all ties: the first four rows
    t = tr.check(g, _send(topo, g, src, dst))
    assert (t["nodes"][1]["in_lat_dev"] < 0).all() and (t["group_nodes"][1]["out_err_dev"] < 0).all() and (t["groups"][1]["lat_dev"] < 0).all()
    _select_all(g, t, lambda n: (0, 1, 4, n + 1), lambda v: (-INF, 0.0, float(np.sort(v)[len(v) // 2])))
    for s, top, sides in _tops(g):
        for side in sides:
            kw = {} if side is None else dict(side=side)
            assert len(top(0, 0.0, by="surge", **kw)[1]) == 0 == len(top(0, 0.0, by="load_up", **kw)[1])
            assert len(top(0, 0.0, by="drop", **kw)[1]) == len(t[s][0]) == len(top(0, 0.0, by="load_down", **kw)[1])


# ---- 8. lifecycle and return codes ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14)
    mk = topo.n_nodes + 8
    P = dict(shift=3, warmup=2, ttl=3, max_entries=700, **FLOORS)
    reads = (g.window_traffic, g.window_node_traffic, g.window_group_traffic, g.window_group_node_traffic)
    ent = lambda s: len(g.traffic_trend_entries(s))                   # noqa: E731
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE                          # off
    for s in ALL:
        assert _rc(g.traffic_trend_entries, s) == engine.SG_ESTATE and _rc(g.traffic_trend_stats, s) == engine.SG_ESTATE
        assert _rc(g.window_traffic_buffer, s) == engine.SG_ESTATE
    for bad in (0, 3, 16):
        assert _rc(g.window_traffic_buffer, bad) == engine.SG_EINVAL and _rc(g.traffic_trend_entries, bad) == engine.SG_EINVAL
        assert _rc(g.traffic_trend_stats, bad) == engine.SG_EINVAL
    assert _rc(g.window_nodes_top_traffic, 1) == engine.SG_ESTATE and _rc(g.window_groups_top_traffic, 1) == engine.SG_ESTATE
    assert _rc(g.window_group_nodes_top_traffic, 1) == engine.SG_ESTATE
    for s in ("nodes", "groups", "group_nodes", ALL):                 # a space needs its rows; the pod edges need nothing
        assert _rc(g.set_traffic_trend, s, **P) == engine.SG_ESTATE
    g.set_traffic_trend("edges", **P)
    assert ent("edges") == 0 and g.traffic_trend_stats("edges").windows == 0
    g.set_nodes()
    g.set_traffic_trend(("edges", "nodes"), **P)                      # needs neither a mean baseline nor K20
    assert _rc(g.set_traffic_trend, ("nodes", "groups"), **P) == engine.SG_ESTATE and ent("nodes") == 0    # refused: the stage stays as it was
    assert _rc(g.set_traffic_trend, 16, **P) == engine.SG_EINVAL and _rc(g.set_traffic_trend, 17, **P) == engine.SG_EINVAL   # unknown space bits
    assert _rc(g.set_traffic_trend, "nodes", **{**P, "shift": 11}) == engine.SG_EINVAL
    assert _rc(g.set_traffic_trend, "nodes", **{**P, "max_entries": (1 << 31) + 1}) == engine.SG_EINVAL
    assert _rc(g.set_traffic_trend, "nodes", **{**P, "load_floor_ns": (1 << 52) + 1}) == engine.SG_EINVAL
    g.set_traffic_trend("nodes", **{**P, "load_floor_ns": 1 << 52, "rate_floor": 0xFFFFFFFF})
    assert _rc(g.traffic_trend_entries, "edges") == engine.SG_ESTATE  # every call replaces the previous setting
    _feed(g, wins[0]); g.flush_window()
    tr = Traffic(g, mk, spaces=("edges", "nodes"), **P)
    assert _rc(g.window_node_traffic) == engine.SG_ESTATE             # the last read window was closed while this baseline was off
    assert _rc(g.window_nodes_top_traffic, 1) == engine.SG_ESTATE and _rc(g.window_traffic_buffer, "nodes") == engine.SG_ESTATE
    _feed(g, wins[1])
    rows = g.flush_window().copy()
    tr.check(g, rows)
    assert _rc(g.window_node_traffic, np.array([len(g.window_nodes())], np.uint32)) == engine.SG_EINVAL
    assert _rc(g.window_traffic, np.array([len(rows)], np.uint32)) == engine.SG_EINVAL
    idx = np.array([3, 0, 3], np.uint32)
    assert g.window_node_traffic(idx).tobytes() == g.window_node_traffic()[idx].tobytes()
    assert g.window_traffic(idx).tobytes() == g.window_traffic()[idx].tobytes()
    assert _rc(g.window_group_traffic) == engine.SG_ESTATE and _rc(g.window_groups_top_traffic, 1) == engine.SG_ESTATE   # that space is not on
    g.set_groups(); g.group_assign(np.arange(mk), _map("blocks", mk, topo.n_pods)); g.set_group_nodes()
    g.set_node_trend(shift=3, warmup=2)
    tr = Traffic(g, mk, **P)                                          # every call starts empty baselines
    assert [ent(s) for s in ALL] == [0, 0, 0, 0]
    _feed(g, wins[2])
    tr.check(g, g.flush_window().copy())
    mean = g.node_trend_entries().tobytes()
    g.set_group_nodes(False)                                          # the workload rows freed underneath: their baseline goes, the others stay
    assert _rc(g.traffic_trend_entries, "group_nodes") == engine.SG_ESTATE and ent("groups") and ent("nodes") and ent("edges")
    g.set_groups()                                                    # any sg_set_groups call frees the group edges' baseline
    assert _rc(g.traffic_trend_entries, "groups") == engine.SG_ESTATE and ent("nodes") and ent("edges")
    assert g.node_trend_entries().tobytes() == mean                   # the mean baseline is not touched
    g.set_node_trend(None); g.set_trend(None)                         # nor does switching a mean baseline touch this stage
    assert ent("nodes") and ent("edges")
    g.set_nodes(False)                                                # the node rows freed: the pod edges stay
    assert _rc(g.traffic_trend_entries, "nodes") == engine.SG_ESTATE and ent("edges")
    g.set_traffic_trend(None)
    assert _rc(g.traffic_trend_entries, "edges") == engine.SG_ESTATE
    g.set_traffic_trend("edges", **P)
    g.set_traffic_trend("edges", None)                                # params None: off
    assert _rc(g.traffic_trend_stats, "edges") == engine.SG_ESTATE
