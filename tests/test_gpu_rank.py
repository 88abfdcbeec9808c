"""K11, the culprit ranking (sg_set_rank / sg_window_rank / sg_window_rank_buffer / sg_window_rank_top / sg_window_rank_select): the
rank rows of every window against the pure-Python reference tests/rank_ref.py run on the same window's rows and node rows — byte
for byte, the contract is integer — on every close path, an engine with it against a twin without it, the selection against
ref_select_rank, and one trace where the ranking names the cause among services with equal scores."""

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _d2h, _engine, _feed, _hip, _path, _rc
from tests.helpers import CLOCK, HostShim
from tests.nodes_ref import nodes_ref
from tests.probe_weights import offsets
from tests.rank_ref import M, rank_ref, ref_select_rank
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


def _check(g, rows, nodes=None, got=None, **params):
    """the last read window's rank rows (or `got`) against the reference over `rows` and the window's node rows; the mass invariant
    on the device result"""
    nodes = g.window_nodes() if nodes is None else nodes
    got = g.window_rank() if got is None else got
    want = rank_ref(rows, nodes, **params)
    assert len(got) == len(nodes) == len(want)
    assert got.tobytes() == want.tobytes()
    if len(got):
        total = sum(int(x) for x in got["rank"])
        assert 0 < total <= M and int(got["rank"].max()) <= M
        assert (got["ref"] == nodes["ref"]).all()
    return got


@pytest.mark.parametrize("seed", ["score", "uniform"])
@pytest.mark.parametrize("iters", [1, 20, 64])
def test_every_window_of_the_churn_is_exact(churn, seed, iters):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes(); g.set_rank(iters=iters, seed=seed)
    n_nodes = set()
    for w in wins:
        _feed(g, w)
        rows = g.flush_window().copy()
        rk = _check(g, rows, iters=iters, seed=seed)
        n_nodes.add(len(rk))
    assert len(n_nodes) > 3 and min(n_nodes) > 100


def test_a_twin_without_it_is_unchanged(churn):
    """edge rows, node rows, edge trend, node trend and vanished lists of an engine with the ranking against a twin without it;
    non-default damping and a seed threshold on the way"""
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(shift=3, warmup=2, ttl=4); x.set_vanished(silent_windows=1, min_seen=1)
        x.set_node_trend(shift=3, warmup=2, ttl=3, max_entries=700)
    p = dict(iters=7, damping_q8=131, seed="score", seed_min_score=0.5)
    g.set_rank(**p)
    for w in wins:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        nodes = g.window_nodes()
        assert nodes.tobytes() == twin.window_nodes().tobytes() == nodes_ref(rows).tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_node_trend().tobytes() == twin.window_node_trend().tobytes()
        assert g.window_vanished().tobytes() == twin.window_vanished().tobytes()
        _check(g, rows, nodes, **p)
    assert g.node_trend_entries().tobytes() == twin.node_trend_entries().tobytes()


def test_warm_delta_and_cold_windows(warm_stream):
    topo, labels, wins = warm_stream
    g = _engine(topo, labels, max_window_events=700_000)
    g.set_nodes(); g.set_rank()
    seen = {}
    for w in wins:
        _feed(g, w)
        s0 = g.stats()
        rows = g.flush_window().copy()
        p = _path(s0, g.stats())
        seen[p] = seen.get(p, 0) + 1
        _check(g, rows)
    assert seen.get("cold", 0) > 0 and seen.get("warm", 0) > 0 and seen.get("delta", 0) > 0, seen


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_k1_variants(churn, variant):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=variant)
    g.set_nodes(); g.set_rank(iters=5)
    for w in wins[:6]:
        _feed(g, w)
        _check(g, g.flush_window().copy(), iters=5)


def test_histogram_engine(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, edge_histogram=True)
    g.set_nodes(); g.set_rank(iters=5, seed="uniform")
    for w in wins[:5]:
        _feed(g, w)
        _check(g, g.flush_window().copy(), iters=5, seed="uniform")


def test_begin_end_view_top_and_index_gather(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    g.set_nodes(); g.set_rank()
    rng = np.random.default_rng(5)
    for i, w in enumerate(wins[:8]):
        _feed(g, w); _feed(twin, w)
        full = twin.flush_window().copy()
        if i % 4 == 0:
            g.flush_begin()
            assert _rc(g.window_rank) == engine.SG_ESTATE                # a flush is open
            assert _rc(g.window_rank_top, 1) == engine.SG_ESTATE
            rows = g.flush_end().copy()
        elif i % 4 == 1:
            rows = g.flush_window_view().copy()
        elif i % 4 == 2:
            g.flush_begin()
            rows = g.flush_end_view().copy()
        else:
            sel, idx, n_edges = g.flush_window_top(3)
            assert n_edges == len(full)
            rows = full
        assert rows.tobytes() == full.tobytes()
        rk = _check(g, rows)
        idx = rng.integers(0, len(rk), 37).astype(np.uint32)
        assert g.window_rank(idx).tobytes() == rk[idx].tobytes()
        assert _rc(g.window_rank, np.array([len(rk)], np.uint32)) == engine.SG_EINVAL


@pytest.mark.parametrize("in_flight", [1, 3, 8])
def test_window_run_in_flight(churn, in_flight):
    """sg_window_run with windows in flight: each slot's rank rows against its own window (the scratch is shared and chained); read
    only after all of a round of slots were enqueued, so that the rankings of several windows are queued behind each other"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    g.set_nodes(); g.set_rank(iters=9)
    one.set_nodes()
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending = []
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        rows = one.flush_window().copy()
        nodes = one.window_nodes()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((rows, nodes, g.rank_buffer(), g.nodes_buffer()))
        if len(pending) == in_flight or i == 8:
            torch.cuda.synchronize()
            for rows, nodes, rp, (np_, cp) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                assert _d2h(hip, np_, cnt, engine.NODE_DTYPE).tobytes() == nodes.tobytes()
                _check(g, rows, nodes, got=_d2h(hip, rp, cnt, engine.RANK_DTYPE), iters=9)
            pending = []


def test_window_run_and_read(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2)
    g.set_nodes(); g.set_rank()
    for w in wins[:4]:
        _feed(g, w)
        g.window_run()
        _check(g, g.window_read().copy())


def _big(topo, labels, max_known, max_edges, **kw):
    g = engine.ServiceGraph(max_known_nodes=max_known, max_edges=max_edges, layers=2, max_labels=256, max_outbound_ips=512,
                            k1_variant=3, warm=True, max_window_events=300_000, max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def test_several_node_ranges_and_slices(churn):
    """max_known_nodes = 40 000 and max_edges = 2^17: plan_rank has 3 node ranges (the labels and outbound IPs are in the last, the
    middle one is unused) and 4 row slices"""
    topo, labels, wins = churn
    g = _big(topo, labels, 40_000, 1 << 17)
    assert (g.window_buffers()[3] + 16383) // 16384 == 3
    g.set_nodes(); g.set_rank()
    kinds = set()
    for w in wins[:5]:
        _feed(g, w)
        rk = _check(g, g.flush_window().copy())
        kinds |= set((rk["ref"] >> 30).tolist())
    assert kinds == {0, 1, 2}


def test_destination_hub():
    """one service called by 24 000 pods (24 000 rows into one accumulator) beside ordinary traffic"""
    topo = replay.make_topology(24_000, 30_000, seed=171, svcs=50)
    ev, labels = replay.make_events(topo, 60_000, seed=172)
    hub = np.zeros(topo.n_pods, dtype=replay.EVENT_DTYPE)
    hub["saddr"] = topo.pod_ips; hub["daddr"] = topo.svc_ips[0]; hub["status"] = 200; hub["protocol"] = replay.PROTO_HTTP
    hub["duration_ns"] = 1_000_000 + 37 * np.arange(len(hub), dtype=np.uint64)
    hub["status"][::3] = 503
    hub["write_time_ns"] = ev["write_time_ns"].max() + np.arange(len(hub), dtype=np.uint64)
    g = _big(topo, labels, topo.n_nodes + 8, 1 << 17)
    g.set_nodes(); g.set_rank()
    for seed in ("score", "uniform"):
        g.set_rank(seed=seed)
        _feed(g, np.concatenate([ev, hub]))
        rows = g.flush_window().copy()
        svc0 = topo.n_pods                                             # node ids: the pods, then the services
        assert int((rows["to_ref"] == svc0).sum()) >= 20_000
        _check(g, rows, seed=seed)


def _check_top(g, nodes, rk, k, t, cap=None):
    sel, rsel, idx, nn = g.window_rank_top(k, t, cap=cap)
    want = ref_select_rank(rk, k, t)
    if cap is not None:
        want = want[:cap]
    assert nn == len(nodes)
    assert idx.tolist() == want.tolist(), (k, t)
    assert sel.tobytes() == nodes[want].tobytes() and rsel.tobytes() == rk[want].tobytes()
    return want


def test_selection_against_the_reference(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes(); g.set_rank()
    checked = 0
    for w in wins[:4]:
        _feed(g, w)
        rows = g.flush_window().copy()
        nodes = g.window_nodes()
        rk = _check(g, rows, nodes)
        n = len(nodes)
        for t in (float("-inf"), 0.0, float(np.median(rk["share"])), float(rk["share"].max())):
            for k in sorted({0, 1, 100, n + 5, engine.SELECT_MAX_K}):
                checked += len(_check_top(g, nodes, rk, k, t)) > 0
        for k in (0, 50):
            _check_top(g, nodes, rk, k, 0.0, cap=10)
        assert len(g.window_rank_top(5, float("nan"))[2]) == 0
    assert checked > 50


def test_device_form_matches_the_host_form(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, windows_in_flight=2)
    g.set_nodes(); g.set_rank()
    hip = _hip()
    cap = 4096
    d_out = torch.zeros(cap * engine.NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:4]]
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:4]):
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        np_, cp = g.nodes_buffer()
        rp = g.rank_buffer()
        torch.cuda.synchronize()
        cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
        nodes, rk = _d2h(hip, np_, cnt, engine.NODE_DTYPE), _d2h(hip, rp, cnt, engine.RANK_DTYPE)
        for k, t in ((0, 0.0), (1, float("-inf")), (100, 0.0), (engine.SELECT_MAX_K, float("-inf")), (0, float(np.median(rk["share"])))):
            g.window_rank_select(k, t, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0)
            torch.cuda.synchronize()
            m = int(d_n.cpu()[0])
            want = ref_select_rank(rk, k, t)
            assert m == len(want), (k, t)
            take = min(m, cap)
            assert d_idx.cpu().numpy()[:take].astype(np.uint32).tolist() == want[:take].tolist()
            assert d_out.cpu().numpy()[: take * engine.NODE_DTYPE.itemsize].tobytes() == nodes[want[:take]].tobytes()
        g.window_rank_select(5, float("-inf"), d_out.data_ptr(), 0, cap, d_n.data_ptr(), 0)      # rows only
        torch.cuda.synchronize()
        want = ref_select_rank(rk, 5)
        assert d_out.cpu().numpy()[: len(want) * engine.NODE_DTYPE.itemsize].tobytes() == nodes[want].tobytes()
    # the host form over a read window selects the same
    _feed(g, wins[4])
    rows = g.flush_window().copy()
    nodes = g.window_nodes()
    rk = _check(g, rows, nodes)
    _check_top(g, nodes, rk, 100, 0.0)


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.set_rank) == engine.SG_ESTATE                         # the rollup is off
    assert _rc(g.window_rank) == engine.SG_ESTATE and _rc(g.rank_buffer) == engine.SG_ESTATE
    assert _rc(g.window_rank_top, 1) == engine.SG_ESTATE
    g.set_nodes()
    assert _rc(g.window_rank) == engine.SG_ESTATE                      # the ranking is off
    for bad in (dict(iters=65), dict(damping_q8=256), dict(seed=2), dict(struct_size=20), dict(reserved=1)):
        assert _rc(g.set_rank, **bad) == engine.SG_EINVAL
    _feed(g, wins[0]); g.flush_window()
    g.set_rank()
    assert _rc(g.window_rank) == engine.SG_ESTATE                      # the read window was closed before it was on
    assert _rc(g.window_rank_top, 1) == engine.SG_ESTATE
    _feed(g, wins[1])
    rows = g.flush_window().copy()
    _check(g, rows)
    assert g._l.sg_window_rank_top(g._h, engine.SELECT_MAX_K + 1, 0.0, None, None, None, 0, None, None) == engine.SG_EINVAL
    assert g._l.sg_window_nodes_top(g._h, 6, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL   # stays: the ranking has its own calls
    _feed(g, wins[2])
    g.flush_begin()
    assert _rc(g.set_rank) == engine.SG_ESTATE and _rc(g.set_rank, None) == engine.SG_ESTATE   # a flush is open
    rows = g.flush_end().copy()
    _check(g, rows)
    g.set_rank(iters=3)                                                # new parameters: the windows from here on
    assert _rc(g.window_rank) == engine.SG_ESTATE
    _feed(g, wins[3])
    _check(g, g.flush_window().copy(), iters=3)
    g.set_rank(None)
    assert _rc(g.window_rank) == engine.SG_ESTATE
    g.set_rank()
    g.set_nodes(False)                                                 # the rollup off takes the ranking with it
    assert _rc(g.window_rank) == engine.SG_ESTATE and _rc(g.set_rank) == engine.SG_ESTATE
    g.set_nodes(True)
    _feed(g, wins[4]); g.flush_window()
    assert _rc(g.window_rank) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_nodes, True) == engine.SG_EINVAL
    assert _rc(g.set_rank) == engine.SG_ESTATE


def test_the_ranking_names_the_cause_where_the_scores_tie():
    """a -> b -> x with every request of all three hops failing (the failure of x echoed up) beside healthy a -> h -> y, under a blob
    whose score is sigmoid(c * err_ratio - c / 2) and nothing else: a, b and x have the SAME node score; the ranking names x"""
    L, c = 2, 8.0
    o = offsets(L)
    blob = np.zeros(weights.weights_count(L), dtype=np.float32)
    blob[o["We"] + 4 * weights.F_HID] = c                              # edge feature 4 (err_ratio) into hidden unit 0
    blob[o["w2"]] = 1.0
    blob[o["b2"]] = -c / 2
    topo = replay.make_topology(16, 20, seed=7)
    a, b, x, h, y = (int(ip) for ip in topo.pod_ips[:5])
    parts = []
    for i, (s, d, status) in enumerate(((a, b, 503), (b, x, 503), (a, h, 200), (h, y, 200))):
        e = np.zeros(40, dtype=replay.EVENT_DTYPE)
        e["saddr"] = s; e["daddr"] = d; e["status"] = status; e["protocol"] = replay.PROTO_HTTP
        e["duration_ns"] = 2_000_000 + 1000 * np.arange(40, dtype=np.uint64)
        e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * (np.arange(40, dtype=np.uint64) + np.uint64(40 * i))
        parts.append(e)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=4096, layers=L, max_labels=16, max_outbound_ips=64)
    g.set_clock(*CLOCK); g.load_weights(blob)
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    g.set_nodes(); g.set_rank()
    g.ingest_bulk(np.concatenate(parts))
    rows = g.flush_window().copy()
    assert len(rows) == 4 and sorted(rows["err_ratio"].tolist()) == [0.0, 0.0, 1.0, 1.0]
    nodes = g.window_nodes()
    rk = _check(g, rows, nodes)
    ra, rb, rx, rh, ry = range(5)                                      # pod i has node id i: the KNOWN ref is the id
    assert nodes["ref"].tolist() == [ra, rb, rx, rh, ry]
    red = nodes["score"][[ra, rb, rx]]
    assert red.view(np.uint32).tolist() == [int(red.view(np.uint32)[0])] * 3 and red[0] > 0.9 > 0.1 > nodes["score"][ry]
    byscore = g.window_nodes_top(3)[1].tolist()
    assert byscore == [ra, rb, rx]                                     # the score alone: a tie, in node order
    for seed in ("score", "uniform"):
        g.set_rank(seed=seed)
        g.ingest_bulk(np.concatenate(parts))
        rows = g.flush_window().copy()
        nodes = g.window_nodes()
        rk = _check(g, rows, nodes, seed=seed)
        sel, rsel, idx, nn = g.window_rank_top(1)
        assert nn == 5 and idx.tolist() == [rx] and sel["ref"][0] == rx and rsel["ref"][0] == rx
        assert rsel["share"][0] > 2 * max(rk["share"][ra], rk["share"][rb])
