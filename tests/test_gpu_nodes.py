"""K9, the node rollup (sg_set_nodes / sg_window_nodes / sg_window_nodes_buffer): every window's node rows against the numpy
reference tests/nodes_ref.py over the rows of the same window, byte for byte, and the rows of an engine with the rollup against a twin
without it, byte for byte.  Every field is an integer sum, an integer max or a max of floats: there is one correct value."""
import ctypes
import threading

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import RUNS, _feed, _hip, _path, _pods_engine
from tests.helpers import CLOCK, HostShim
from tests.nodes_ref import nodes_ref

pytestmark = pytest.mark.gpu

ME = 1 << 15


def _engine(topo, labels, layers=2, *, variant=0, max_edges=ME, **kw):
    if variant == 0:                                                  # the 8-byte-record path with the warm state kept
        kw.setdefault("warm", True)
        variant = 3
    elif variant == 3:
        kw.setdefault("warm", False)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=256,
                            max_outbound_ips=512, k1_variant=variant, max_window_events=kw.pop("max_window_events", 300_000),
                            max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(layers))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def _check(g, rows):
    want = nodes_ref(rows)
    got = g.window_nodes()
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    return got


def _rc(call, *a):
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(*a)
    return ei.value.rc


@pytest.fixture(scope="module")
def churn():
    """12 windows over one topology: whole groups of edges missing from some windows and coming back, raw outbound IPs, Host
    labels, reversed events and open-connection (alive-only) records"""
    topo = replay.make_topology(300, 6000, seed=81)
    ev, labels = replay.make_events(topo, 360_000, seed=82, mixed=True, with_raw_outbound=True, with_reverse=True)
    rng = np.random.default_rng(83)
    al = np.zeros(3000, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
    pick = rng.random(len(al))
    al["daddr"] = np.where(pick < 0.5, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))],
                           np.where(pick < 0.8, topo.pod_ips[rng.integers(0, topo.n_pods, len(al))], 0x5DB8D800 + rng.integers(0, 40, len(al)))).astype(np.uint32)
    group = ((ev["saddr"].astype(np.uint64) * 2654435761 + ev["daddr"].astype(np.uint64) * 40503) >> 7) % 6
    wins = []
    for i in range(12):
        part = ev[i * 30_000:(i + 1) * 30_000]
        gp = group[i * 30_000:(i + 1) * 30_000]
        keep = (gp != (i % 6)) & ((gp != 5) | (i < 4) | (i > 8))        # group i % 6 absent for one window; group 5 for five
        a = al[rng.random(len(al)) < 0.3]
        wins.append(np.concatenate([part[keep], a]))
    return topo, labels, wins


@pytest.fixture(scope="module")
def warm_stream():
    """windows without raw outbound IPs on one topology, three draws of its events with the same Host labels: a first window (cold),
    a subset of it (warm), another draw (delta: edges the kept set lacks), the first again (warm), the third draw (delta)"""
    topo = replay.make_topology(400, 30_000, seed=91)
    (e0, labels), (e1, _), (e2, _) = (replay.make_events(topo, 150_000, seed=92 + k, fixed_labels=True) for k in range(3))
    wins = [e0, e0[::3], e1, e0, e2, e1[::2]]
    return topo, labels, wins


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("layers", [1, 2])
def test_every_k1_variant_matches_the_reference_and_changes_no_row(churn, variant, layers):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels, layers, variant=variant), _engine(topo, labels, layers, variant=variant)
    g.set_nodes()
    for w in wins[:5]:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()        # the rollup changes no row
        n = _check(g, rows)
        assert len(n) > 100


def test_churn_stream_through_every_window_path(churn, warm_stream):
    seen = {}
    for topo, labels, wins in (churn, warm_stream):
        g, twin = _engine(topo, labels, max_window_events=700_000), _engine(topo, labels, max_window_events=700_000)
        g.set_nodes()
        for w in wins:
            _feed(g, w); _feed(twin, w)
            s0 = g.stats()
            rows = g.flush_window().copy()
            p = _path(s0, g.stats())
            assert rows.tobytes() == twin.flush_window().tobytes()
            n = _check(g, rows)
            seen[p] = seen.get(p, 0) + 1
            types = set((n["ref"] >> 30).tolist())
            assert 0 in types
    assert seen.get("cold", 0) > 0 and seen.get("warm", 0) > 0 and seen.get("delta", 0) > 0, seen


def test_outbound_ips_labels_reversed_and_alive_only_rows(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes()
    _feed(g, wins[0])
    rows = g.flush_window()
    n = _check(g, rows)
    types = n["ref"] >> 30
    assert (types == 1).sum() > 0 and (types == 2).sum() > 0                # Host labels and raw outbound IPs
    assert (rows["count"] == 0).sum() > 0 and n["in_alive"].sum() == rows["alive"].sum() == n["out_alive"].sum() > 0
    assert n["out_edges"].sum() == n["in_edges"].sum() == len(rows)


def test_histogram_engine(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels, variant=2, edge_histogram=True), _engine(topo, labels, variant=2, edge_histogram=True)
    g.set_nodes()
    for w in wins[:3]:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        _check(g, rows)


def test_split_flush_with_the_next_window_fed_beside_it(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes()

    def feed_threads(e, threads=4):
        parts = np.array_split(np.arange(0, len(e), 1 << 14), threads)

        def run(ix):
            for i in ix:
                while g.ingest(e[i:i + (1 << 14)]) != 0:
                    pass
        ths = [threading.Thread(target=run, args=(p,)) for p in parts]
        for t in ths:
            t.start()
        return ths
    _feed(g, wins[0])
    for i in range(4):
        g.flush_begin()
        assert _rc(g.window_nodes) == engine.SG_ESTATE                # the open flush rolls up into the same buffer
        ths = feed_threads(wins[i + 1])
        rows = g.flush_end().copy()
        for t in ths:
            t.join()
        _check(g, rows)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_window_run_in_flight_through_the_device_buffer(churn, in_flight):
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    g.set_nodes()
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:6]):
        _feed(one, w)
        rows = one.flush_window().copy()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        rp = g.rows_buffer()
        npp, cp = g.nodes_buffer()
        torch.cuda.synchronize()
        got_rows = np.zeros(len(rows), dtype=replay.EDGE_OUT_DTYPE)
        assert hip.hipMemcpy(got_rows.ctypes.data, ctypes.c_void_p(rp), got_rows.nbytes, 2) == 0
        assert got_rows.tobytes() == rows.tobytes()
        cnt = np.zeros(1, dtype=np.uint64)
        assert hip.hipMemcpy(cnt.ctypes.data, ctypes.c_void_p(cp), 8, 2) == 0
        got = np.zeros(int(cnt[0]), dtype=engine.NODE_DTYPE)
        assert hip.hipMemcpy(got.ctypes.data, ctypes.c_void_p(npp), got.nbytes, 2) == 0
        want = nodes_ref(rows)
        assert len(got) == len(want) > 100
        assert got.tobytes() == want.tobytes()


def _hub_engine(n_pods, max_edges):
    g = engine.ServiceGraph(max_known_nodes=n_pods + 16, max_edges=max_edges, layers=2, max_labels=16, max_outbound_ips=64,
                            max_window_events=4 * n_pods, max_batch=1 << 16, k1_variant=1)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(2))
    for i in range(n_pods):
        g.upsert_pod(replay.POD_IP_BASE + i, i)
    g.upsert_service(0x0B000001, n_pods)
    return g


def test_hub_destination_and_a_source_across_many_chunks():
    """119 999 pods call one service (a destination with 119 999 in-edges, one node of one range) and pod 0 calls every other pod
    (an out-run of 119 999 rows: ~60 chunks of k9_out).  Pods 1 .. P-1 are alike, so their rows to the service
    score alike: the service's worst row is the first of many equal maxima."""
    P = 120_000
    g = _hub_engine(P, 1 << 18)
    g.set_nodes()
    ev = np.zeros(2 * (P - 1), dtype=replay.EVENT_DTYPE)
    ev["saddr"][:P - 1] = replay.POD_IP_BASE + np.arange(1, P)
    ev["daddr"][:P - 1] = 0x0B000001
    ev["saddr"][P - 1:] = replay.POD_IP_BASE
    ev["daddr"][P - 1:] = replay.POD_IP_BASE + np.arange(1, P)
    ev["protocol"] = 1
    ev["status"] = 200
    ev["duration_ns"] = 250_000
    ev["write_time_ns"] = CLOCK[0] + 1000
    g.ingest_bulk(ev)
    rows = g.flush_window()
    assert len(rows) == 2 * (P - 1)
    n = _check(g, rows)
    hub = n[n["ref"] == P][0]
    src = n[n["ref"] == 0][0]
    assert hub["in_edges"] == P - 1 and src["out_edges"] == P - 1
    to_hub = rows["to_ref"] == P
    assert (rows["score"][to_hub] == hub["in_score_max"]).sum() > 1000   # many equal maxima: the lowest row is the worst
    assert hub["in_worst_row"] == np.flatnonzero(to_hub & (rows["score"] == hub["in_score_max"]))[0]


@pytest.fixture(scope="module")
def wide():
    """4200 pods, pod i with node id i, no groups: pod 5 is the caller of the long run, pods 0..4 come before it in row order"""
    topo, g, mk = _pods_engine(n_pods=4200)
    g.set_nodes()
    return topo, g


@pytest.mark.parametrize("front,D", RUNS)
def test_out_side_runs_at_the_span_and_chunk_boundaries(wide, front, D):
    topo, g = wide
    f = np.arange(front)                                              # pods 0..4 call `front` pods between them
    src = np.concatenate([f % 5, np.full(D, 5), [50, 50, 51]])
    dst = np.concatenate([60 + f // 5, np.arange(D) + 100, [7, 8, 7]])
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = topo.pod_ips[dst]
    e["status"] = 200; e["protocol"] = replay.PROTO_HTTP; e["duration_ns"] = 1_000_000
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    g.ingest_bulk(e)
    rows = g.flush_window().copy()
    n = _check(g, rows)
    assert len(rows) == front + D + 3
    assert rows["from_ref"][front] == 5 == rows["from_ref"][front + D - 1] and rows["from_ref"][front - 1] == 4 and rows["from_ref"][front + D] == 50
    w = n[n["ref"] == 5][0]
    assert w["out_edges"] == D and w["out_count"] == D and w["in_edges"] == 0


def test_empty_window_and_states(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.window_nodes) == engine.SG_ESTATE                    # off
    assert _rc(g.nodes_buffer) == engine.SG_ESTATE
    g.set_nodes()
    assert _rc(g.window_nodes) == engine.SG_ESTATE                    # no window closed with the rollup on yet
    g.set_nodes()                                                     # (on while on: nothing changes)
    assert len(g.flush_window()) == 0
    assert len(g.window_nodes()) == 0                                 # a window without rows
    _feed(g, wins[0])
    g.flush_begin()
    assert _rc(g.set_nodes, False) == engine.SG_ESTATE                # a flush is open
    assert _rc(g.set_nodes, True) == engine.SG_ESTATE
    _check(g, g.flush_end().copy())
    rc = g._l.sg_set_nodes(g._h, 2)
    assert rc == engine.SG_EINVAL


def test_switching_on_and_off_between_windows(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for i, w in enumerate(wins[:7]):
        on = i in (0, 1, 4, 6)
        if on:
            g.set_nodes(True)
        else:
            g.set_nodes(False)
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        if on:
            _check(g, rows)
        else:
            assert _rc(g.window_nodes) == engine.SG_ESTATE            # off
            g.set_nodes(True)
            assert _rc(g.window_nodes) == engine.SG_ESTATE            # that window was closed while the rollup was off
            g.set_nodes(False)


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_nodes, True) == engine.SG_EINVAL
    assert _rc(g.window_nodes) == engine.SG_ESTATE


def test_top1_row_is_its_nodes_worst_row(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    g.set_nodes()
    for w in wins[:4]:
        _feed(g, w); _feed(twin, w)
        sel, idx, n_edges = g.flush_window_top(1)
        rows = twin.flush_window()
        assert n_edges == len(rows) and len(idx) == 1
        nodes = _check(g, rows)
        r, s = int(idx[0]), sel["score"][0]
        src = nodes[nodes["ref"] == sel["from_ref"][0]][0]
        dst = nodes[nodes["ref"] == sel["to_ref"][0]][0]
        assert src["score"] == s == src["out_score_max"] and src["out_worst_row"] == r
        assert dst["score"] == s == dst["in_score_max"] and dst["in_worst_row"] == r


def test_config3_full_size():
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_nodes()
    for w in (ev, ev[: len(ev) // 3], ev):
        g.ingest_bulk(w)
        rows = g.flush_window()
        assert len(rows) > 500_000
        n = _check(g, rows)
        assert len(n) > 10_000 and n["out_edges"].max() > 2048            # some out-run crosses a chunk
