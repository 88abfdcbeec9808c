"""K21, the tail baselines (sg_set_quantile_trend / sg_window_node_quantile_trend / sg_window_group_quantile_trend /
sg_window_group_node_quantile_trend / sg_window_quantile_trend_buffer / sg_quantile_trend_entries / sg_quantile_trend_stats_get and
the three _top_tail selections): the tail rows, the whole baseline and its statistics of every space after every window against
the references of tests/quantile_trend_ref.py — byte for byte — run on the same engine's own node rows, group edges, workload rows,
outbound IPs and quantile tables of that window (K20's tables are held to tests/quantile_ref.py by tests/test_gpu_quantiles.py,
and once more here).  Engines are small (max_edges <= 2^15); the shapes are those of tests/test_gpu_node_trend.py and
tests/test_gpu_group_trend.py: K8's walk takes one workgroup per 2048 merged elements."""
import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import _d2h, _engine, _feed, _hip, _map, _pairs, _pods_engine, _rc, _send
from tests.group_trend_ref import ref_select_groups
from tests.helpers import G
from tests.node_trend_ref import ref_select_nodes
from tests import quantile_ref as qr
from tests.quantile_trend_ref import GroupTailRef, NodeTailRef, WorkloadTailRef
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

NO = engine.NO_GROUP
ALL = ("nodes", "groups", "group_nodes")
STATS = ("windows", "entries", "inserted", "expired", "dropped")
PARAMS = dict(shift=3, warmup=2, ttl=3, max_entries=700)             # a small ttl, and a capacity the churn overflows
DEFAULT = (500, 990)
EIGHT = (1, 250, 500, 750, 900, 990, 999, 1000)
INF = float("inf")

#: per space: the entity rows, the quantile read, the tail read
READS = dict(nodes=("window_nodes", "window_node_quantiles", "window_node_quantile_trend"),
             groups=("window_groups", "window_group_quantiles", "window_group_quantile_trend"),
             group_nodes=("window_group_nodes", "window_group_node_quantiles", "window_group_node_quantile_trend"))


def _stages(g, gmap=None, spaces=ALL, permille=DEFAULT):
    g.set_nodes(); g.set_groups()
    if gmap is not None:
        g.group_assign(np.arange(len(gmap)), gmap)
    g.set_group_nodes()
    g.set_quantiles(spaces, permille)


class Tail:
    """the references of one engine's tail baselines and the check of the last read window against them"""

    def __init__(self, g, mk, spaces=ALL, permille=DEFAULT, tracked=990, ml=256, mob=512, **params):
        ncap = g.window_buffers()[3]
        nc = min(mk + mk + ml + mob, 2 * g.max_edges)                 # (max_groups defaults to max_known_nodes)
        self.spaces, self.qi = spaces, permille.index(tracked)
        make = dict(nodes=lambda: NodeTailRef(ncap, **params), groups=lambda: GroupTailRef(g.max_edges, **params),
                    group_nodes=lambda: WorkloadTailRef(nc, **params))
        self.ref = {s: make[s]() for s in spaces}
        g.set_quantile_trend(spaces, tracked, **params)

    def want(self, g, space, ents=None, quant=None):
        rows, quants, _ = READS[space]
        ents = getattr(g, rows)() if ents is None else ents
        q = (getattr(g, quants)() if quant is None else quant)[..., self.qi]
        return ents, self.ref[space].window(ents, q, g.outbound_ips())

    def check(self, g):
        out = {}
        for s in self.spaces:
            ents, want = self.want(g, s)
            got = getattr(g, READS[s][2])()
            assert len(got) == len(ents) and got.dtype == want.dtype
            for f in got.dtype.names:
                assert got[f].tobytes() == want[f].tobytes(), (s, f)
            ref = self.ref[s]
            assert g.quantile_trend_entries(s).tobytes() == ref.entries.tobytes(), s
            st = g.quantile_trend_stats(s)
            assert tuple(getattr(st, k) for k in STATS) == tuple(ref.stats[k] for k in STATS), s
            out[s] = (ents, got)
        return out


def _twin_reads(g):
    calls = ["window_nodes", "window_groups", "window_group_nodes", "window_group_perm", "window_hist", "window_node_hist",
             "window_node_quantiles", "window_group_hist", "window_group_quantiles", "window_group_node_hist", "window_group_node_quantiles",
             "window_node_trend", "window_group_trend", "window_group_node_trend", "node_trend_entries", "group_trend_entries",
             "group_node_trend_entries"]
    return {c: getattr(g, c)().tobytes() for c in calls}


# ---- 1. the churn: exact, a twin without the stage unchanged, the identities with the mean baselines ---------------------------------
@pytest.mark.parametrize("kind", ["none", "blocks"])
def test_churn_is_exact_a_twin_is_unchanged_and_the_error_half_is_the_mean_baselines(churn, kind):
    """entities that come and go, OBIP nodes whose list index changes, alive-only entities, ttl 3 and a capacity the churn
    overflows.  Both engines keep the three mean baselines with the same parameters from the same window: every other output is
    the twin's byte for byte, and the tail rows' err_dev / seen and the entries' err_mean, err_dev, n, last are the mean
    baselines' (same keys, same counts, same error samples: the same merge).  "none": the workload space is the node space."""
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    gmap = _map(kind, mk, topo.n_pods)
    g, twin = (_engine(topo, labels, variant=2, edge_histogram=True) for _ in range(2))
    for x in (g, twin):
        _stages(x, gmap)
        x.set_node_trend(**PARAMS); x.set_group_trend(**PARAMS); x.set_group_node_trend(**PARAMS)
    tail = Tail(g, mk, **PARAMS)
    seen = 0
    for i, w in enumerate(wins[:9]):
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        a, b = _twin_reads(g), _twin_reads(twin)
        for c in a:
            assert a[c] == b[c], c
        t = tail.check(g)
        if i == 1:                                                    # K20's tables once more against their own reference
            nodes, Q = t["nodes"][0], g.window_node_quantiles()
            assert Q.tobytes() == qr.node_quantiles(qr.fold_nodes(g.window_hist(), rows, nodes), nodes, DEFAULT).tobytes()
        for s, mean, ent in (("nodes", g.window_node_trend(), g.node_trend_entries()), ("group_nodes", g.window_group_node_trend(), g.group_node_trend_entries())):
            for f in ("in_err_dev", "out_err_dev", "in_seen", "out_seen"):
                assert t[s][1][f].tobytes() == mean[f].tobytes(), (s, f)
            te = g.quantile_trend_entries(s)
            for f in ("from_key", "to_key", "err_mean", "err_dev", "n", "last"):
                assert te[f].tobytes() == ent[f].tobytes(), (s, f)
        mean, ent, te = g.window_group_trend(), g.group_trend_entries(), g.quantile_trend_entries("groups")
        for f in ("err_dev", "windows_seen"):
            assert t["groups"][1][f].tobytes() == mean[f].tobytes(), f
        for f in ("from_key", "to_key", "err_mean", "err_dev", "n", "last"):
            assert te[f].tobytes() == ent[f].tobytes(), f
        if kind == "none":
            assert t["group_nodes"][1].tobytes() == t["nodes"][1].tobytes()
            wk, nk = g.quantile_trend_entries("group_nodes"), g.quantile_trend_entries("nodes")
            assert np.array_equal(wk["from_key"], nk["from_key"] + np.uint64(1 << 32))    # the key's type shift, nothing else
            for f in ("to_key", "lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last"):
                assert wk[f].tobytes() == nk[f].tobytes(), f
        seen += int((t["nodes"][1]["in_lat_dev"] != 0).sum())
    assert seen > 0
    assert tail.ref["nodes"].stats["dropped"] > 0 and tail.ref["nodes"].stats["expired"] > 0


# ---- 2. several workgroups ----------------------------------------------------------------------------------------------------------------
def test_default_capacities_across_workgroups(churn, warm_stream):
    """the default capacities: 4 x ncap + 2 x ncap merged elements of the node space are at least four K8 workgroups, 2 x max_edges +
    max_edges of the group edges 48: every thread's span is a few elements, and spans cross workgroups.  (The 8-byte-record engine;
    an engine with the edge histogram keeps no warm state, so there is one window path.)"""
    for (topo, labels, wins), n in ((warm_stream, 5), (churn, 4)):
        g = _engine(topo, labels, max_obip=1024, max_window_events=700_000, edge_histogram=True)
        mk = topo.n_nodes + 8
        _stages(g, _map("blocks", mk, topo.n_pods))
        tail = Tail(g, mk, mob=1024, shift=2, warmup=1, ttl=5)
        ncap = g.window_buffers()[3]
        assert (6 * ncap + 2047) // 2048 >= 4 and (3 * g.max_edges + 2047) // 2048 == 48
        for w in wins[:n]:
            _feed(g, w)
            g.flush_window()
            t = tail.check(g)
        assert len(t["groups"][0]) > 256 and (t["groups"][1]["lat_dev"] != 0).any()
        assert tail.ref["groups"].cap == 2 * g.max_edges and tail.ref["nodes"].cap == 4 * ncap


# ---- 3. n_q 1 and 8, the tracked per-mille first, last and in the middle; k1_variant 1 and 2 -------------------------------------------
@pytest.mark.parametrize("variant,permille,tracked", [(1, (990,), 990), (2, EIGHT, 1), (1, EIGHT, 1000), (2, EIGHT, 750)],
                         ids=["one", "first", "last", "middle"])
def test_quantile_sets_and_k1_variants(churn, variant, permille, tracked):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=variant, edge_histogram=True)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods), permille=permille)
    tail = Tail(g, mk, permille=permille, tracked=tracked, **PARAMS)
    for w in wins[:5]:
        _feed(g, w)
        g.flush_window()
        t = tail.check(g)
    assert (t["nodes"][1]["in_base_mean_us"] != 0).any()


# ---- 4. constructed windows: the boundaries, the side mapping, a rollout --------------------------------------------------------------
@pytest.fixture()
def small():
    topo, g, mk = _pods_engine(n_pods=140, edge_histogram=True)
    gmap = np.full(mk, NO, np.uint32); gmap[:8] = 0                   # workload 0 = pods 0 .. 7
    _stages(g, gmap)
    return topo, g, mk


def test_empty_single_first_and_expired_windows(small):
    topo, g, mk = small
    tail = Tail(g, mk, ml=16, mob=64, shift=1, warmup=1, ttl=2)
    none = np.zeros(0, np.int64)
    _send(topo, g, none, none)                                        # the first window: B = 0, E = 0
    t = tail.check(g)
    assert all(len(t[s][1]) == 0 and len(g.quantile_trend_entries(s)) == 0 and g.quantile_trend_stats(s).windows == 1 for s in ALL)
    _send(topo, g, [20], [21], dur=3_000_000)                         # B = 0, a single group edge: two node rows
    t = tail.check(g)
    assert len(t["groups"][1]) == 1 and len(g.quantile_trend_entries("groups")) == 1 and len(g.quantile_trend_entries("nodes")) == 2
    _send(topo, g, [20], [21], dur=3_000_000)
    t = tail.check(g)
    assert t["groups"][1]["windows_seen"].tolist() == [1] and t["groups"][1]["base_mean_us"][0] > 0
    _send(topo, g, [20], [21], alive=[True])                          # an alive-only entity: rows, no refresh
    t = tail.check(g)
    assert len(t["groups"][1]) == 1 and t["groups"][1]["lat_dev"][0] == 0 and g.quantile_trend_stats("groups").entries == 1
    for _ in range(2):
        _send(topo, g, none, none)                                    # ttl 2: everything expires
        tail.check(g)
    assert all(g.quantile_trend_stats(s).entries == 0 and g.quantile_trend_stats(s).expired > 0 for s in ALL)
    src, dst = _pairs(30, 200, 3)
    _send(topo, g, src + 20, dst + 20)                                # a window after everything expired
    t = tail.check(g)
    assert all((t[s][1][f] == 0).all() for s, f in (("nodes", "in_seen"), ("groups", "windows_seen"), ("group_nodes", "out_seen")))


def test_the_side_mapping(small):
    """pod 30 is called slowly (8 ms) and calls quickly (1 ms): its in-side quantile differs from its out-side one, and the
    entry of key (nk, 0) — the IN side — holds 1000 x the table's side [1], the entry of (nk, 1) the table's side [0]"""
    topo, g, mk = small
    tail = Tail(g, mk, ml=16, mob=64, shift=1, warmup=1)
    for w in range(3):
        _send(topo, g, [31, 32, 30, 30], [30, 30, 40, 41], dur=[8_000_000, 8_000_000, 1_000_000, 1_000_000])
        t = tail.check(g)
        nodes, Q = t["nodes"][0], g.window_node_quantiles()
        k = int(np.flatnonzero(nodes["ref"] == 30)[0])
        q_out, q_in = int(Q[k, 0, 1]), int(Q[k, 1, 1])
        assert q_in >= 4 * q_out > 0
        e = g.quantile_trend_entries("nodes")
        mine = e[e["from_key"] == 30]
        assert mine["to_key"].tolist() == [0, 1] and mine["lat_mean"].tolist() == [1000.0 * q_in, 1000.0 * q_out]
        row = t["nodes"][1][k]
        if w:
            assert row["in_base_mean_us"] == np.float32(q_in) and row["out_base_mean_us"] == np.float32(q_out)
            assert row["in_lat_dev"] == 0 and row["out_lat_dev"] == 0
    # the in side jumps several octaves, the out side stays: only in_lat_dev moves
    _send(topo, g, [31, 32, 30, 30], [30, 30, 40, 41], dur=[64_000_000, 64_000_000, 1_000_000, 1_000_000])
    row = tail.check(g)["nodes"][1][k]
    assert row["in_lat_dev"] > 1000 and row["out_lat_dev"] == 0
    wrow = g.window_group_node_quantile_trend()[g.window_group_nodes()["ref"] == 30][0]
    assert wrow.tobytes() == row.tobytes()                            # pod 30 is ungrouped: its workload row is its node row


def test_a_rollout_keeps_the_workload_tail_baseline(small):
    """every pod of workload 0 replaced (pods 0 .. 3 leave, 4 .. 7 take their traffic): the node space starts new entries, the
    workload space keeps the tail baseline of workload 0"""
    topo, g, mk = small
    tail = Tail(g, mk, ml=16, mob=64, shift=1, warmup=2)
    old, new, dst = np.repeat(np.arange(0, 4), 3), np.repeat(np.arange(4, 8), 3), np.tile(np.arange(20, 23), 4)
    for w in range(4):
        _send(topo, g, old, dst, dur=2_000_000)
        tail.check(g)
    _send(topo, g, new, dst, dur=2_000_000)
    t = tail.check(g)
    gn, wt = t["group_nodes"]
    k = int(np.flatnonzero(gn["ref"] == G(0))[0])
    assert wt["out_seen"][k] == 4 and wt["out_base_mean_us"][k] > 0
    nodes, nt = t["nodes"]
    assert (nt["out_seen"][np.isin(nodes["ref"], np.arange(4, 8))] == 0).all()


# ---- 5. every close path ----------------------------------------------------------------------------------------------------------------
def test_every_close_path(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    g.set_trend(shift=3, warmup=1)                                    # (for the _top_by flush)
    tail = Tail(g, mk, **PARAMS)
    for i, w in enumerate(wins[:8]):
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_node_quantile_trend, g.window_group_quantile_trend, g.window_group_node_quantile_trend,
                         g.set_quantile_trend, g.window_nodes_top_tail, g.window_groups_top_tail, g.window_group_nodes_top_tail):
                assert _rc(call, *((1,) if "top" in call.__name__ else ())) == engine.SG_ESTATE     # a flush is open
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
        elif i == 6:
            g.flush_window_top(2, by="lat_dev")                       # sg_flush_window_top_by
        else:
            g.flush_begin(); g.flush_end_top(2)
        tail.check(g)


# ---- 6. three windows in flight -----------------------------------------------------------------------------------------------------------
def test_window_run_three_in_flight_through_the_device_buffers(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True, windows_in_flight=3)
    one = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    for x in (g, one):
        _stages(x, gmap)
    tail = Tail(one, mk, **PARAMS)
    g.set_quantile_trend(ALL, 990, **PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(wins[:6]):
        _feed(one, w)
        one.flush_window()
        t = tail.check(one)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((t, [g.window_quantile_trend_buffer(s) for s in ALL]))
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
        assert g.quantile_trend_entries(s).tobytes() == tail.ref[s].entries.tobytes()


# ---- 7. the selections ----------------------------------------------------------------------------------------------------------------------
def test_the_tail_selections(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    g.set_node_trend(shift=3, warmup=1); g.set_group_trend(shift=3, warmup=1); g.set_group_node_trend(shift=3, warmup=1)
    tail = Tail(g, mk, shift=3, warmup=1)
    for w in wins[:3]:
        _feed(g, w)
        g.flush_window()
        t = tail.check(g)
    for s, top, plain in (("nodes", g.window_nodes_top_tail, g.window_nodes_top), ("group_nodes", g.window_group_nodes_top_tail, g.window_group_nodes_top)):
        ents, tr = t[s]
        assert (tr["in_lat_dev"] != 0).any()
        for by in engine.NSEL_BY:
            v = ents["score"] if by == "score" else tr["in_lat_dev" if by == "new" else by]
            mid = float(np.sort(v)[len(v) // 2])
            for k in (0, 1, 7, len(ents) + 5):
                for thr in (-INF, mid, INF):
                    want = ref_select_nodes(ents, tr, by, k, thr)
                    rows, idx, n = top(k, thr, by=by)
                    assert n == len(ents) and idx.tolist() == want.tolist(), (s, by, k, thr)
                    assert rows.tobytes() == ents[want].tobytes()
        # the tail rows are the source, not the mean baseline's: the two orders differ
        assert top(7, by="in_lat_dev")[1].tolist() != plain(7, by="in_lat_dev")[1].tolist()
        assert top(0, by="score")[0].tobytes() == plain(0, by="score")[0].tobytes()
    ge, tr = t["groups"]
    for by in engine.SEL_BY:
        v = ge["score_max"] if by == "score" else tr["lat_dev" if by == "new" else by]
        mid = float(np.sort(v)[len(v) // 2])
        for k in (0, 1, 7, len(ge) + 5):
            for thr in (-INF, mid, INF):
                want = ref_select_groups(ge, tr, by, k, thr)
                rows, idx, n = g.window_groups_top_tail(k, thr, by=by)
                assert n == len(ge) and idx.tolist() == want.tolist(), (by, k, thr)
                assert rows.tobytes() == ge[want].tobytes()
    assert g.window_groups_top_tail(7)[1].tolist() != g.window_groups_top(7, by="lat_dev")[1].tolist()
    assert g._l.sg_window_nodes_top_tail(g._h, 6, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL      # by > SG_NSEL_NEW
    assert g._l.sg_window_groups_top_tail(g._h, 4, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL     # by > SG_SEL_NEW
    assert g._l.sg_window_group_nodes_top_tail(g._h, 0, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL


# ---- 8. lifecycle and return codes ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    mk = topo.n_nodes + 8
    reads = (g.window_node_quantile_trend, g.window_group_quantile_trend, g.window_group_node_quantile_trend)
    assert _rc(g.set_quantile_trend, "nodes") == engine.SG_EINVAL    # no per-mille set yet: 990 is not among them
    g.set_nodes(); g.set_quantiles("nodes")
    assert _rc(g.set_quantile_trend, "groups") == engine.SG_ESTATE   # a space K20 has not on
    assert _rc(g.set_quantile_trend, ALL) == engine.SG_ESTATE
    assert _rc(g.set_quantile_trend, 8) == engine.SG_EINVAL and _rc(g.set_quantile_trend, 9) == engine.SG_EINVAL   # unknown space bits
    assert _rc(g.set_quantile_trend, "nodes", 991) == engine.SG_EINVAL      # not among {500, 990}
    assert _rc(g.set_quantile_trend, "nodes", 990, shift=11) == engine.SG_EINVAL
    assert _rc(g.set_quantile_trend, "nodes", 990, max_entries=(1 << 31) + 1) == engine.SG_EINVAL
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE                          # off
    for s in ALL:
        assert _rc(g.quantile_trend_entries, s) == engine.SG_ESTATE and _rc(g.quantile_trend_stats, s) == engine.SG_ESTATE
        assert _rc(g.window_quantile_trend_buffer, s) == engine.SG_ESTATE
    for bad in (0, 3, 8):
        assert _rc(g.window_quantile_trend_buffer, bad) == engine.SG_EINVAL and _rc(g.quantile_trend_entries, bad) == engine.SG_EINVAL
        assert _rc(g.quantile_trend_stats, bad) == engine.SG_EINVAL
    assert _rc(g.window_nodes_top_tail, 1) == engine.SG_ESTATE and _rc(g.window_groups_top_tail, 1) == engine.SG_ESTATE
    assert _rc(g.window_nodes_top_tail, 1, by="score") == engine.SG_ESTATE   # the plain selection serves the score; the tail one needs the stage
    _feed(g, wins[0]); g.flush_window()
    tail = Tail(g, mk, spaces=("nodes",), tracked=500, **PARAMS)
    assert _rc(g.window_node_quantile_trend) == engine.SG_ESTATE      # the last read window was closed while the stage was off
    assert _rc(g.window_nodes_top_tail, 1) == engine.SG_ESTATE and _rc(g.window_quantile_trend_buffer, "nodes") == engine.SG_ESTATE
    assert len(g.quantile_trend_entries("nodes")) == 0 and g.quantile_trend_stats("nodes").windows == 0
    _feed(g, wins[1]); g.flush_window()
    tail.check(g)
    assert _rc(g.window_node_quantile_trend, np.array([len(g.window_nodes())], np.uint32)) == engine.SG_EINVAL
    idx = np.array([3, 0, 3], np.uint32)
    assert g.window_node_quantile_trend(idx).tobytes() == g.window_node_quantile_trend()[idx].tobytes()
    assert _rc(g.window_group_quantile_trend) == engine.SG_ESTATE     # that space is not on
    g.set_quantile_trend("nodes", 990, **PARAMS)                      # every call starts empty baselines
    assert len(g.quantile_trend_entries("nodes")) == 0
    g.set_quantiles("nodes", (990, 500))                              # ANY sg_set_quantiles switches the stage off: the index may have moved
    assert _rc(g.quantile_trend_entries, "nodes") == engine.SG_ESTATE and _rc(g.window_node_quantile_trend) == engine.SG_ESTATE
    g.set_groups(); g.group_assign(np.arange(mk), _map("blocks", mk, topo.n_pods)); g.set_group_nodes()
    g.set_quantiles(ALL)
    g.set_node_trend(**PARAMS)
    tail = Tail(g, mk, **PARAMS)
    _feed(g, wins[2]); g.flush_window()
    tail.check(g)
    mean = g.node_trend_entries().tobytes()
    g.set_group_nodes(False)                                          # a K20 space freed underneath: its tail baseline goes, the others stay
    assert _rc(g.quantile_trend_entries, "group_nodes") == engine.SG_ESTATE
    assert len(g.quantile_trend_entries("groups")) and len(g.quantile_trend_entries("nodes"))
    g.set_groups()                                                    # any sg_set_groups call
    assert _rc(g.quantile_trend_entries, "groups") == engine.SG_ESTATE and len(g.quantile_trend_entries("nodes"))
    assert g.node_trend_entries().tobytes() == mean                   # the mean baseline is not touched
    g.set_node_trend(None)                                            # nor does it touch the tail baseline
    assert len(g.quantile_trend_entries("nodes"))
    g.set_quantile_trend(None)
    assert _rc(g.quantile_trend_entries, "nodes") == engine.SG_ESTATE
    g.set_quantile_trend("nodes", 990, **PARAMS)
    g.set_quantile_trend("nodes", 990, None)                          # params None: off
    assert _rc(g.quantile_trend_stats, "nodes") == engine.SG_ESTATE
    g.set_quantile_trend("nodes", 990, **PARAMS)
    g.set_nodes(False)
    assert _rc(g.quantile_trend_entries, "nodes") == engine.SG_ESTATE
