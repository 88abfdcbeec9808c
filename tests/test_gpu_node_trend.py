"""K10, the per-node baselines (sg_set_node_trend / sg_window_node_trend / sg_window_node_trend_buffer / sg_node_trend_entries): the
node trend rows and the whole node baseline after every window against the numpy reference tests/node_trend_ref.py, run on the node
rows and outbound IPs of the same windows — byte for byte, as K8's — and an engine with it against a twin without it."""

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import PARAMS, _d2h, _engine, _feed, _hip, _ncap, _path, _rc
from tests.helpers import CLOCK, HostShim
from tests.node_trend_ref import NodeTrendRef
from tests.nodes_ref import nodes_ref
from tests.traces import _drift
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

ME = 1 << 15


def _check(g, ref, nodes, trend=None):
    want = ref.window(nodes, g.outbound_ips())
    got = g.window_node_trend() if trend is None else trend
    assert len(got) == len(nodes)
    assert got.tobytes() == want.tobytes()
    assert g.node_trend_entries().tobytes() == ref.entries.tobytes()
    s = g.node_trend_stats()
    assert (s.windows, s.entries, s.inserted, s.expired, s.dropped) == tuple(ref.stats[k] for k in ("windows", "entries", "inserted", "expired", "dropped"))
    return want


def test_churn_is_exact_and_a_twin_without_it_is_unchanged(churn):
    """variant 0 warm engine over the churn: node trend rows, entries and stats against the reference; edge rows, node rows, edge
    trend rows and vanished lists against a twin with the node trend off"""
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(shift=3, warmup=2, ttl=4); x.set_vanished(silent_windows=1, min_seen=1)
    g.set_node_trend(**PARAMS)
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    obs, dev_seen = set(), 0
    for w in wins:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        nodes = g.window_nodes()
        assert nodes.tobytes() == twin.window_nodes().tobytes() == nodes_ref(rows).tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_vanished().tobytes() == twin.window_vanished().tobytes()
        t = _check(g, ref, nodes)
        obs.add(g.outbound_ips().tobytes())
        dev_seen += int((t["in_lat_dev"] != 0).sum() + (t["out_err_dev"] != 0).sum())
    assert len(obs) > 3 and dev_seen > 0
    assert ref.stats["dropped"] > 0 and ref.stats["expired"] > 0


def test_warm_delta_and_cold_windows_across_workgroups(churn, warm_stream):
    """every window path of the variant-0 engine; the default capacity (4 x ncap) and max_obip = 1024 give plan_node_trend at
    least four workgroups (B + 2N spread over them: spans cross workgroups)"""
    seen = {}
    for topo, labels, wins in (warm_stream, churn):
        g = _engine(topo, labels, max_obip=1024, max_window_events=700_000)
        g.set_nodes(); g.set_node_trend(shift=2, warmup=1, ttl=5)
        ncap = _ncap(g)
        assert (4 * ncap + 2 * ncap + 2047) // 2048 >= 4
        ref = NodeTrendRef(ncap, shift=2, warmup=1, ttl=5)
        for w in wins:
            _feed(g, w)
            s0 = g.stats()
            g.flush_window()
            seen[_path(s0, g.stats())] = seen.get(_path(s0, g.stats()), 0) + 1
            _check(g, ref, g.window_nodes())
    assert seen.get("cold", 0) > 0 and seen.get("warm", 0) > 0 and seen.get("delta", 0) > 0, seen


@pytest.mark.parametrize("variant", [1, 2])
def test_other_k1_variants(churn, variant):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=variant)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    for w in wins[:8]:
        _feed(g, w)
        g.flush_window()
        _check(g, ref, g.window_nodes())


def test_begin_end_and_index_gather(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    rng = np.random.default_rng(5)
    for w in wins[:8]:
        _feed(g, w)
        g.flush_begin()
        assert _rc(g.window_node_trend) == engine.SG_ESTATE             # a flush is open
        g.flush_end()
        nodes = g.window_nodes()
        t = _check(g, ref, nodes)
        idx = rng.integers(0, len(nodes), 37).astype(np.uint32)
        assert g.window_node_trend(idx).tobytes() == t[idx].tobytes()
        assert _rc(g.window_node_trend, np.array([len(nodes)], np.uint32)) == engine.SG_EINVAL


@pytest.mark.parametrize("in_flight", [1, 3])
def test_window_run_in_flight_against_one_call_flushes(churn, in_flight):
    """sg_window_run with 1 or 3 windows in flight: the device buffer of each window equals the reference (and so a one-call engine's)"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    for x in (g, one):
        x.set_nodes(); x.set_node_trend(**PARAMS)
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        one.flush_window()
        nodes = one.window_nodes()
        want = one.window_node_trend()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        tp = g.node_trend_buffer()
        np_, cp = g.nodes_buffer()
        torch.cuda.synchronize()
        cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
        assert _d2h(hip, np_, cnt, engine.NODE_DTYPE).tobytes() == nodes.tobytes()
        got = _d2h(hip, tp, cnt, engine.NODE_TREND_DTYPE)
        assert got.tobytes() == want.tobytes() == ref.window(nodes, one.outbound_ips()).tobytes()
    assert g.node_trend_entries().tobytes() == one.node_trend_entries().tobytes() == ref.entries.tobytes()


def test_window_run_and_read(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    for w in wins[:8]:
        _feed(g, w)
        g.window_run()
        g.window_read()
        _check(g, ref, g.window_nodes())


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.set_node_trend) == engine.SG_ESTATE                  # the rollup is off
    assert _rc(g.window_node_trend) == engine.SG_ESTATE
    assert _rc(g.node_trend_entries) == engine.SG_ESTATE and _rc(g.node_trend_stats) == engine.SG_ESTATE
    assert _rc(g.node_trend_buffer) == engine.SG_ESTATE
    g.set_nodes()
    assert _rc(g.set_node_trend, shift=11) == engine.SG_EINVAL
    assert _rc(g.set_node_trend, max_entries=(1 << 31) + 1) == engine.SG_EINVAL
    assert _rc(g.set_node_trend, struct_size=36) == engine.SG_EINVAL
    g.set_node_trend(**PARAMS)
    assert _rc(g.window_node_trend) == engine.SG_ESTATE               # no window closed with it on yet
    assert len(g.node_trend_entries()) == 0 and g.node_trend_stats().windows == 0
    _feed(g, wins[0]); g.flush_window()
    assert len(g.window_node_trend()) == len(g.window_nodes()) > 0 and len(g.node_trend_entries()) > 0
    g.set_trend(); g.set_trend(None)                                  # the edge trend does not touch it
    assert g.node_trend_stats().windows == 1
    _feed(g, wins[1])
    g.flush_begin()
    assert _rc(g.set_node_trend, None) == engine.SG_ESTATE            # a flush is open
    assert _rc(g.set_node_trend) == engine.SG_ESTATE
    g.flush_end()
    assert g.node_trend_stats().windows == 2
    g.set_node_trend(**PARAMS)                                        # re-enabling starts empty
    assert len(g.node_trend_entries()) == 0 and g.node_trend_stats().windows == 0
    assert _rc(g.window_node_trend) == engine.SG_ESTATE               # the last read window was closed before
    _feed(g, wins[2]); g.flush_window()
    ref = NodeTrendRef(_ncap(g), **PARAMS)
    _check(g, ref, g.window_nodes())
    g.set_node_trend(None)
    assert _rc(g.window_node_trend) == engine.SG_ESTATE
    g.set_node_trend(**PARAMS)
    g.set_nodes(False)                                                # the rollup off takes the node trend with it
    assert _rc(g.node_trend_stats) == engine.SG_ESTATE
    g.set_nodes(True)
    assert _rc(g.node_trend_stats) == engine.SG_ESTATE
    _feed(g, wins[3]); g.flush_window()
    assert _rc(g.window_node_trend) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_nodes, True) == engine.SG_EINVAL
    assert _rc(g.set_node_trend) == engine.SG_ESTATE


def test_config3_two_windows():
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_nodes(); g.set_node_trend(warmup=1)
    ref = NodeTrendRef(_ncap(g), warmup=1)
    rng = np.random.default_rng(3)
    for i in range(2):
        g.ingest_bulk(_drift(ev, i + 1, rng))
        g.flush_window()
        nodes = g.window_nodes()
        assert len(nodes) > 10_000
        t = _check(g, ref, nodes)
    assert (t["in_lat_dev"] > 0).sum() > 1000
