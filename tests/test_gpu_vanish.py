"""K8's vanished list (sg_set_vanished / sg_window_vanished / sg_window_vanished_buffer): every window's list against the numpy
reference tests/vanish_ref.py run on the rows and outbound IPs of the same windows, and everything else the engine returns against a
twin engine with the list off.  Every comparison is exact: bytes of the list, the count, the rows, the trend rows and entries."""
import ctypes

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _feed, _hip, _rc, _trend_engine as _engine
from tests.helpers import CLOCK, HostShim
from tests.traces import trend_churn as churn  # noqa: F401  (the churn trace: groups of edges missing for 1 and 5 windows)
from tests.trend_ref import TrendRef
from tests.vanish_ref import NO_ROW, VanishRef

pytestmark = pytest.mark.gpu

ME = 1 << 15
PARAMS = dict(shift=3, warmup=2, ttl=6)


def _check(g, vref, rows, got=None):
    tr, want, n = vref.window(rows, g.outbound_ips())
    lst, cnt = g.window_vanished(with_count=True) if got is None else got
    assert cnt == n
    assert lst.tobytes() == want.tobytes()
    return tr, want, n


@pytest.mark.parametrize("silent", [1, 3])
@pytest.mark.parametrize("min_seen", [1, 0])
def test_churn_lists_are_exact_and_nothing_else_changes(churn, silent, min_seen):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    g.set_trend(**PARAMS); twin.set_trend(**PARAMS)
    g.set_vanished(silent_windows=silent, min_seen=min_seen)
    vref = VanishRef(TrendRef(ME, **PARAMS), silent_windows=silent, min_seen=min_seen)
    total, with_row = 0, 0
    for w in wins:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        tr, want, n = _check(g, vref, rows)
        assert g.window_trend().tobytes() == twin.window_trend().tobytes() == tr.tobytes()
        assert g.trend_entries().tobytes() == twin.trend_entries().tobytes() == vref.trend.entries.tobytes()
        total += n; with_row += int((want["row"] != NO_ROW).sum())
    assert total > 50
    if silent == 1:
        assert with_row > 0                                           # an alive-only row behind a silent entry


def test_max_rows_below_the_windows_count(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_trend(**PARAMS); g.set_vanished(min_seen=1, max_rows=7)
    vref = VanishRef(TrendRef(ME, **PARAMS), min_seen=1, max_rows=7)
    big = 0
    for w in wins[:6]:
        _feed(g, w)
        _, _, n = _check(g, vref, g.flush_window())
        big += n > 7
    assert big > 0


@pytest.mark.parametrize("kind", ["v1_l1", "v2_l2", "no_warm", "histogram", "begin_end", "view", "top"])
def test_every_close_path(churn, kind):
    topo, labels, wins = churn
    kw = dict(v1_l1=dict(variant=1, layers=1), v2_l2=dict(variant=2, layers=2), no_warm=dict(variant=3, warm=False),
              histogram=dict(variant=2, edge_histogram=True)).get(kind, {})
    g, twin = _engine(topo, labels, **kw), _engine(topo, labels, **kw)
    for e in (g, twin):
        e.set_trend(**PARAMS)
    g.set_vanished(min_seen=1)
    vref = VanishRef(TrendRef(ME, **PARAMS), min_seen=1)
    total = 0
    for w in wins[:8]:
        _feed(g, w); _feed(twin, w)
        want = twin.flush_window()
        if kind == "begin_end":
            g.flush_begin(); rows = g.flush_end()
        elif kind == "view":
            rows = g.flush_window_view().copy()
        elif kind == "top":
            _, _, ne = g.flush_window_top(10)
            assert ne == len(want)
            rows = want
        else:
            rows = g.flush_window()
        assert rows.tobytes() == want.tobytes()
        total += _check(g, vref, want)[2]
    assert total > 0


def test_window_run_two_in_flight_and_the_buffer(churn):
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=2), _engine(topo, labels)
    for e in (g, one):
        e.set_trend(**PARAMS)
    g.set_vanished(min_seen=1, max_rows=500)
    vref = VanishRef(TrendRef(ME, **PARAMS), min_seen=1, max_rows=500)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    total = 0
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        rows = one.flush_window().copy()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        lp, cp = g.vanished_buffer()
        torch.cuda.synchronize()
        cnt = np.zeros(1, np.uint64)
        assert hip.hipMemcpy(cnt.ctypes.data, ctypes.c_void_p(cp), 8, 2) == 0
        lst = np.zeros(min(int(cnt[0]), 500), dtype=engine.VANISHED_DTYPE)
        if len(lst):
            assert hip.hipMemcpy(lst.ctypes.data, ctypes.c_void_p(lp), lst.nbytes, 2) == 0
        total += _check(one, vref, rows, got=(lst, int(cnt[0])))[2]
    assert total > 0
    assert g.trend_entries().tobytes() == vref.trend.entries.tobytes()


def test_window_run_sharded_world_1(churn):
    if not engine.RcclComm.probe():
        pytest.skip("RCCL not loadable in this process")
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2)
    g.set_trend(**PARAMS); g.set_vanished(min_seen=1)
    vref = VanishRef(TrendRef(ME, **PARAMS), min_seen=1)
    comm = engine.RcclComm(0, 1, 0, lambda b: b)
    total = 0
    try:
        for w in wins[:6]:
            _feed(g, w)
            g.window_run_sharded(comm)
            total += _check(g, vref, g.window_read())[2]
    finally:
        comm.close()
    assert total > 0


def test_states_invalid_parameters_and_set_trend_resets(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.set_vanished) == engine.SG_ESTATE                    # the trend is off
    g.set_trend(**PARAMS)
    for call in (g.window_vanished, g.vanished_buffer):
        assert _rc(call) == engine.SG_ESTATE                          # the list is off
    for bad in (dict(silent_windows=6), dict(silent_windows=9), dict(struct_size=12), dict(max_rows=2 * ME + 1)):
        assert _rc(g.set_vanished, **bad) == engine.SG_EINVAL
    g.set_vanished(silent_windows=5)
    assert _rc(g.window_vanished) == engine.SG_ESTATE                 # no window closed with the list on yet
    vref = VanishRef(TrendRef(ME, **PARAMS), silent_windows=5)
    _feed(g, wins[0])
    g.flush_begin()
    assert _rc(g.window_vanished) == engine.SG_ESTATE                 # a flush is open
    assert _rc(g.set_vanished) == engine.SG_ESTATE
    _check(g, vref, g.flush_end())
    g.set_trend(**PARAMS)                                             # any set_trend switches the list off
    assert _rc(g.window_vanished) == engine.SG_ESTATE
    _feed(g, wins[1]); g.flush_window()                               # closed with the list off
    g.set_vanished(min_seen=1)
    assert _rc(g.window_vanished) == engine.SG_ESTATE
    ref = TrendRef(ME, **PARAMS)
    ref.entries = g.trend_entries(); ref.w = 1                        # the baseline after the window closed with the list off
    vref = VanishRef(ref, min_seen=1)
    for w in wins[2:5]:
        _feed(g, w)
        _check(g, vref, g.flush_window())
    g.set_vanished(None)
    assert _rc(g.window_vanished) == engine.SG_ESTATE


def test_config3_full_size_window_pair_with_a_dropped_group():
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_trend(warmup=1); g.set_vanished()
    vref = VanishRef(TrendRef(1_250_000, warmup=1))
    group = ((ev["saddr"].astype(np.uint64) * 2654435761 + ev["daddr"].astype(np.uint64) * 40503) >> 7) % 8
    counts = []
    for w in (ev, ev[group != 3]):
        g.ingest_bulk(w)
        rows = g.flush_window()
        assert len(rows) > 400_000
        counts.append(_check(g, vref, rows)[2])
    assert counts[0] == 0 and counts[1] > 1000
