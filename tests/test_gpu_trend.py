"""K8, the per-edge baselines (sg_set_trend / sg_window_trend / sg_window_trend_buffer / sg_trend_entries): the trend rows and the
whole baseline after every window against the numpy reference tests/trend_ref.py, run on the rows and outbound IPs of the same
windows.  The state is fp64 without division and the outputs are correctly rounded fp64 divisions, so every comparison is exact:
bytes of the trend rows, bytes of the entry dump, the counts."""
import ctypes

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _feed, _hip, _trend_engine as _engine
from tests.helpers import CLOCK, HostShim
from tests.traces import trend_churn as churn  # noqa: F401  (the fixture)
from tests.trend_ref import TrendRef, row_keys, strictly_ascending

pytestmark = pytest.mark.gpu

ME = 1 << 15
PARAMS = dict(shift=3, warmup=2, ttl=3)


def _check(g, ref, rows, trend=None):
    want = ref.window(rows, g.outbound_ips())
    got = g.window_trend() if trend is None else trend
    assert len(got) == len(rows)
    assert got.tobytes() == want.tobytes()
    ent = g.trend_entries()
    assert ent.tobytes() == ref.entries.tobytes()
    s = g.trend_stats()
    assert (s.windows, s.entries, s.inserted, s.expired, s.dropped) == tuple(ref.stats[k] for k in ("windows", "entries", "inserted", "expired", "dropped"))
    return want


def test_multi_window_churn_is_exact_and_rows_are_unchanged(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    g.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    reentries, seen_expired, alive_only, obip_keys = 0, False, 0, 0
    for i, w in enumerate(wins):
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()        # the trend changes no row
        fk, tk = row_keys(rows, g.outbound_ips())
        assert strictly_ascending(fk, tk)                             # the design's premise: canonical order = key order
        obip_keys += int(((fk >> np.uint64(32)) == 2).sum() + ((tk >> np.uint64(32)) == 2).sum())
        alive_only += int((rows["count"] == 0).sum())
        out = _check(g, ref, rows)
        if i >= 7:                                                    # edges that expired (or were never seen) and came back
            reentries += int(((out["windows_seen"] == 0) & (rows["count"] > 0)).sum())
        seen_expired |= ref.stats["expired"] > 0
    assert seen_expired and obip_keys > 0 and alive_only > 0 and reentries > 0
    assert (g.window_trend()["lat_dev"] != 0).sum() > 100 and (g.window_trend()["windows_seen"] >= 4).sum() > 100


@pytest.mark.parametrize("kind", ["v1_l1", "v1_l2", "v2_l1", "v2_l2", "v0_l1", "histogram", "no_warm"])
def test_every_path_gives_the_same_trend_bytes(churn, kind):
    topo, labels, wins = churn
    kw = dict(v1_l1=dict(variant=1, layers=1), v1_l2=dict(variant=1, layers=2), v2_l1=dict(variant=2, layers=1),
              v2_l2=dict(variant=2, layers=2), v0_l1=dict(layers=1), histogram=dict(variant=2, edge_histogram=True),
              no_warm=dict(variant=3, warm=False))[kind]
    g = _engine(topo, labels, **kw)
    g.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    for w in wins[:8]:
        _feed(g, w)
        _check(g, ref, g.flush_window())


def test_begin_end_and_top_with_an_index(churn):
    topo, labels, wins = churn
    a, b = _engine(topo, labels), _engine(topo, labels)
    a.set_trend(**PARAMS); b.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    for i, w in enumerate(wins[:7]):
        _feed(a, w); _feed(b, w)
        a.flush_begin()
        rows = a.flush_end()
        want = _check(a, ref, rows)
        sel, idx, n = b.flush_window_top(50)                          # the selection's positions: only those trend rows cross PCIe
        assert n == len(rows) and len(idx) == min(50, n)
        assert b.window_trend(index=idx).tobytes() == want[idx].tobytes()
        assert b.window_trend(index=idx[::-1]).tobytes() == want[idx[::-1]].tobytes()
        assert b.trend_entries().tobytes() == ref.entries.tobytes()
    with pytest.raises(engine.ServiceGraphError) as ei:
        b.window_trend(index=np.array([n], dtype=np.uint32))          # beyond the window's rows
    assert ei.value.rc == engine.SG_EINVAL


@pytest.mark.parametrize("in_flight", [2, 4])
def test_window_run_in_flight_against_one_slot(churn, in_flight):
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    g.set_trend(**PARAMS); one.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        rows = one.flush_window().copy()
        want = _check(one, ref, rows)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        rp, tp = g.rows_buffer(), g.trend_buffer()
        torch.cuda.synchronize()
        got_rows = np.zeros(len(rows), dtype=replay.EDGE_OUT_DTYPE)
        got = np.zeros(len(rows), dtype=engine.TREND_DTYPE)
        assert hip.hipMemcpy(got_rows.ctypes.data, ctypes.c_void_p(rp), got_rows.nbytes, 2) == 0
        assert hip.hipMemcpy(got.ctypes.data, ctypes.c_void_p(tp), got.nbytes, 2) == 0
        assert got_rows.tobytes() == rows.tobytes()
        assert got.tobytes() == want.tobytes()
    assert g.trend_entries().tobytes() == ref.entries.tobytes()


def test_window_run_sharded_world_1(churn):
    if not engine.RcclComm.probe():
        pytest.skip("RCCL not loadable in this process")
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2)
    g.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    comm = engine.RcclComm(0, 1, 0, lambda b: b)
    try:
        for w in wins[:6]:
            _feed(g, w)
            g.window_run_sharded(comm)
            rows = g.window_read()
            _check(g, ref, rows)
    finally:
        comm.close()


def test_small_spans_straddle_matched_pairs(churn):
    """At 2^15 edges the plan gives 48 workgroups of 256 threads for at most 3 x 2^15 merged elements: a window of a few thousand
    rows and entries has spans of one or two elements, so nearly every (entry, row) pair is split between two threads and many
    between two workgroups.  A small baseline capacity gives few workgroups and long spans: both must agree with the reference."""
    topo, labels, wins = churn
    wgs = min(1024, -(-(2 * ME + ME) // 2048))
    g = _engine(topo, labels)
    g.set_trend(**PARAMS)
    ref = TrendRef(ME, **PARAMS)
    for w in wins[:5]:
        _feed(g, w)
        rows = g.flush_window()
        _check(g, ref, rows)
        T = len(rows) + ref.stats["entries"]
        assert -(-T // (wgs * 256)) <= 2
    g2 = _engine(topo, labels)
    g2.set_trend(max_entries=1000, **PARAMS)                          # 1 workgroup: spans of ~ T / 256
    ref2 = TrendRef(ME, max_entries=1000, **PARAMS)
    for w in wins[:5]:
        _feed(g2, w)
        _check(g2, ref2, g2.flush_window())


@pytest.mark.parametrize("ttl", [1, 3])
def test_ttl(churn, ttl):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_trend(shift=2, warmup=1, ttl=ttl)
    ref = TrendRef(ME, shift=2, warmup=1, ttl=ttl)
    for w in wins[:8]:
        _feed(g, w)
        _check(g, ref, g.flush_window())
    assert ref.stats["expired"] > 0


def test_capacity_below_one_windows_edges(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_trend(max_entries=700, **PARAMS)
    ref = TrendRef(ME, max_entries=700, **PARAMS)
    _feed(g, wins[0])
    rows = g.flush_window()
    live = rows["count"] > 0
    assert live.sum() > 700
    _check(g, ref, rows)
    s = g.trend_stats()
    assert (s.windows, s.entries, s.inserted, s.expired, s.dropped) == (1, 700, 700, 0, int(live.sum()) - 700)
    fk, tk = row_keys(rows[live][:700], g.outbound_ips())            # the first 700 live rows in key order
    ent = g.trend_entries()
    assert np.array_equal(ent["from_key"], fk) and np.array_equal(ent["to_key"], tk)
    for w in wins[1:5]:
        _feed(g, w)
        _check(g, ref, g.flush_window())
    assert g.trend_stats().entries <= 700


def test_states_invalid_parameters_and_reenabling(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    for call in (g.window_trend, g.trend_entries, g.trend_stats, g.trend_buffer):
        with pytest.raises(engine.ServiceGraphError) as ei:
            call()
        assert ei.value.rc == engine.SG_ESTATE
    for bad in (dict(shift=11), dict(struct_size=32), dict(reserved=1), dict(max_entries=(1 << 31) + 1)):
        with pytest.raises(engine.ServiceGraphError) as ei:
            g.set_trend(**bad)
        assert ei.value.rc == engine.SG_EINVAL
    with pytest.raises(engine.ServiceGraphError):
        g.window_trend()                                              # a refused set_trend leaves it off
    g.set_trend(**PARAMS)
    assert len(g.trend_entries()) == 0 and g.trend_stats().windows == 0
    _feed(g, wins[0])
    g.flush_begin()
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_trend(**PARAMS)                                         # a flush is open
    assert ei.value.rc == engine.SG_ESTATE
    ref = TrendRef(ME, **PARAMS)
    ref.window(g.flush_end(), g.outbound_ips())                       # the window of the refused call is trend window 1
    _feed(g, wins[1]); _check(g, ref, g.flush_window())
    assert g.trend_stats().windows == 2
    g.set_trend(None)
    with pytest.raises(engine.ServiceGraphError):
        g.trend_entries()
    _feed(g, wins[2]); rows_off = g.flush_window()                    # off: nothing is kept
    g.set_trend(**PARAMS)                                             # re-enabled: empty again, w starts at 1
    assert len(g.trend_entries()) == 0 and g.trend_stats().windows == 0
    ref = TrendRef(ME, **PARAMS)
    for w in wins[3:6]:
        _feed(g, w)
        out = _check(g, ref, g.flush_window())
    assert len(rows_off) > 0 and out["windows_seen"].max() == 2


def test_config3_full_size():
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_trend(warmup=1)
    ref = TrendRef(1_250_000, warmup=1)
    for w in (ev, ev[: len(ev) // 3], ev):
        g.ingest_bulk(w)
        rows = g.flush_window()
        assert len(rows) > 500_000
        _check(g, ref, rows)
    assert ref.stats["entries"] > 500_000
