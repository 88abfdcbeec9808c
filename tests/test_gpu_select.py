"""K7, the selection (sg_flush_window_top / sg_flush_end_top / sg_window_select): the selected rows against a numpy reference over
the rows of a TWIN engine — same config, same events, closed with the plain sg_flush_window.  A selection moves rows and computes
nothing, so every comparison is exact: row bytes, indices and counts."""
import ctypes
import threading

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _feed, _hip
from tests.helpers import CLOCK, HostShim
from tests.select_by_ref import ref_select

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _engine(nodes, max_edges, layers, *, variant=0, w=None, **kw):
    if variant == 0:                                                  # the 8-byte-record path with the warm state kept
        kw.setdefault("warm", True)
        variant = 3
    g = engine.ServiceGraph(max_known_nodes=nodes, max_edges=max_edges, layers=layers, max_labels=kw.pop("max_labels", 256),
                            max_outbound_ips=kw.pop("max_outbound_ips", 512), k1_variant=variant, **kw)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(layers) if w is None else w)
    return g


def _twins(topo, labels, layers, **kw):
    a, b = _engine(topo.n_nodes + 8, 1 << 15, layers, **kw), _engine(topo.n_nodes + 8, 1 << 15, layers, **kw)
    for g in (a, b):
        HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return a, b


def _check(rows, idx, n_edges, want_rows, k, min_score, cap=None):
    sel = ref_select(want_rows, k, min_score)
    assert n_edges == len(want_rows)
    m = len(sel) if cap is None else min(len(sel), cap)
    assert len(rows) == len(idx) == m
    assert np.array_equal(idx, sel[:m])
    assert rows.tobytes() == want_rows[sel[:m]].tobytes()


@pytest.fixture(scope="module")
def trace():
    topo = replay.make_topology(300, 9000, seed=71)
    ev, labels = replay.make_events(topo, 400_000, seed=72, mixed=True, with_raw_outbound=True)
    return topo, ev, labels


CONFIGS = [(v, l) for v in (0, 1, 2) for l in (1, 2)]


@pytest.mark.parametrize("variant,layers", CONFIGS)
def test_identity_selection_returns_every_row_in_canonical_order(trace, variant, layers):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, layers, variant=variant, max_window_events=300_000, max_batch=1 << 14)
    for w in (ev[:100_000], ev[100_000:300_000]):
        _feed(a, w); _feed(b, w)
        rows, idx, n = a.flush_window_top(0, NEG_INF)
        want = b.flush_window()
        assert n == len(want) > 1000 and rows.tobytes() == want.tobytes()
        assert np.array_equal(idx, np.arange(len(want), dtype=np.uint32))
        assert np.array_equal(a.outbound_ips(), b.outbound_ips())


@pytest.mark.parametrize("variant,layers", CONFIGS)
def test_top_k_equals_the_reference(trace, variant, layers):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, layers, variant=variant, max_window_events=300_000, max_batch=1 << 14)
    w = ev[:60_000]
    _feed(b, w); first = b.flush_window().copy()
    E = len(first)
    assert 1000 < E and E + 5 <= engine.SELECT_MAX_K
    median = float(np.median(first["score"]))
    _feed(a, w); rows, idx, n = a.flush_window_top(1000, median)
    _check(rows, idx, n, first, 1000, median)
    for k in (1, 7, 1000, 16384, E + 5):
        for ms in (NEG_INF, median):
            _feed(a, w); _feed(b, w)
            rows, idx, n = a.flush_window_top(k, ms)
            want = b.flush_window()
            _check(rows, idx, n, want, k, ms)
            assert len(rows) == min(k, int((want["score"] >= np.float32(ms)).sum()))


def test_all_ties_keep_canonical_order(trace):
    topo, ev, labels = trace
    W = np.zeros(weights.weights_count(2), dtype=np.float32)
    a, b = _twins(topo, labels, 2, max_window_events=300_000, max_batch=1 << 14, w=W)
    w = ev[:80_000]
    for k in (1, 7, 1000, 5000):
        _feed(a, w); _feed(b, w)
        rows, idx, n = a.flush_window_top(k, NEG_INF)
        want = b.flush_window()
        assert len(np.unique(want["score"])) == 1                   # every score equal: the tie rule alone decides
        assert np.array_equal(idx, np.arange(min(k, len(want)), dtype=np.uint32))
        assert rows.tobytes() == want[:k].tobytes()


def test_threshold_mode_gives_the_candidates_in_canonical_order(trace):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, 2, max_window_events=300_000, max_batch=1 << 14)
    w = ev[:100_000]
    _feed(b, w); ref = b.flush_window().copy()
    t = float(np.quantile(ref["score"], 0.3))
    _feed(a, w); _feed(b, w)
    rows, idx, n = a.flush_window_top(0, t)
    want = b.flush_window()
    _check(rows, idx, n, want, 0, t)
    assert 0 < len(rows) < len(want) and np.all(np.diff(idx.astype(np.int64)) > 0)
    top = float(np.nextafter(want["score"].max(), np.float32(np.inf)))
    _feed(a, w); _feed(b, w)
    rows, idx, n = a.flush_window_top(0, top)
    assert len(rows) == 0 and n == len(b.flush_window()) > 0


def test_edge_cases_empty_window_short_cap_and_k_too_large(trace):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, 2, max_window_events=300_000, max_batch=1 << 14)
    rows, idx, n = a.flush_window_top(100, NEG_INF)                   # empty window
    assert n == 0 and len(rows) == 0 and len(b.flush_window()) == 0
    w = ev[:100_000]
    for k, cap in ((1000, 10), (0, 25)):                              # cap < n_selected: cap rows, the full count
        _feed(a, w); _feed(b, w)
        out = np.zeros(cap, dtype=replay.EDGE_OUT_DTYPE); ix = np.zeros(cap, dtype=np.uint32)
        ns, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
        a._ck(a._l.sg_flush_window_top(a._h, 0, k, NEG_INF, out.ctypes.data, ix.ctypes.data, cap, ctypes.byref(ns), ctypes.byref(ne)))
        want = b.flush_window()
        sel = ref_select(want, k, NEG_INF)
        assert ns.value == len(sel) > cap and ne.value == len(want)
        assert np.array_equal(ix, sel[:cap]) and out.tobytes() == want[sel[:cap]].tobytes()
    _feed(a, w); _feed(b, w)
    with pytest.raises(engine.ServiceGraphError) as ei:
        a.flush_window_top(engine.SELECT_MAX_K + 1, NEG_INF)
    assert ei.value.rc == engine.SG_EINVAL
    with pytest.raises(engine.ServiceGraphError) as ei:
        a.flush_end_top(engine.SELECT_MAX_K + 1, NEG_INF)
    assert ei.value.rc == engine.SG_EINVAL
    assert a.flush_window().tobytes() == b.flush_window().tobytes()   # nothing was closed by the refused calls
    assert a.stats().windows == b.stats().windows


def _stats(g):
    s = g.stats()
    return {f: getattr(s, f) for f, _ in engine.SgStats._fields_ if f != "ingest_waits"}


@pytest.mark.parametrize("variant", [0, 1])
def test_selection_leaves_the_engine_as_a_plain_flush_does(variant):
    topo = replay.make_topology(400, 30_000, seed=81)
    ev, labels = replay.make_events(topo, 700_000, seed=82, mixed=True)
    a, b = _twins(topo, labels, 2, variant=variant, max_window_events=400_000, max_batch=1 << 14)
    # windows over more and more of the trace: later ones bring edges the earlier ones lacked (delta windows on the warm engine)
    wins = [ev[:30_000], ev[30_000:60_000], ev[60_000:260_000], ev[260_000:660_000]]
    for i, w in enumerate(wins):
        _feed(a, w); _feed(b, w)
        want = b.flush_window()
        if i % 2 == 0:
            rows, idx, n = a.flush_window_top(500, NEG_INF)
            _check(rows, idx, n, want, 500, NEG_INF)
        else:
            assert a.flush_window().tobytes() == want.tobytes()
        assert _stats(a) == _stats(b), i
        assert np.array_equal(a.outbound_ips(), b.outbound_ips())
    if variant == 0:
        st = b.stats()
        assert st.windows_warm + st.windows_cold + st.windows_plain > 0


def test_split_flush_selects_the_closed_window_while_the_next_one_is_fed(trace):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, 2, max_window_events=300_000, max_batch=1 << 14)
    wins = [ev[:120_000], ev[120_000:250_000], ev[250_000:400_000]]
    want = []
    for w in wins:
        _feed(b, w); want.append(b.flush_window().copy())

    def feed_threads(e, threads=4):
        parts = np.array_split(np.arange(0, len(e), 1 << 14), threads)
        def run(ix):
            for i in ix:
                while a.ingest(e[i:i + (1 << 14)]) != 0:
                    pass
        ths = [threading.Thread(target=run, args=(p,)) for p in parts]
        for t in ths: t.start()
        return ths
    feed_threads(wins[0], 1)[0].join()
    for i in range(3):
        a.flush_begin()
        ths = feed_threads(wins[i + 1]) if i + 1 < 3 else []
        rows, idx, n = a.flush_end_top(1000, NEG_INF)
        for t in ths: t.join()
        _check(rows, idx, n, want[i], 1000, NEG_INF)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_window_select_on_the_device(trace, in_flight):
    import torch
    topo, ev, labels = trace
    g = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=300_000, max_batch=1 << 14, windows_in_flight=in_flight)
    b = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=300_000, max_batch=1 << 14)
    for e in (g, b):
        HostShim().apply(e, topo.k8s_ops()); e.set_label_count(len(labels))
    hip = _hip()
    wins = [ev[:100_000], ev[100_000:250_000], ev[250_000:400_000]]
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins]
    cap = 2000
    d_out = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for i, w in enumerate(wins):
        k, ms = ((1000, NEG_INF), (0, 0.5), (16384, NEG_INF))[i]
        _feed(b, w); want = b.flush_window()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        ptr = g.rows_buffer()
        g.window_select(k, ms, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0)
        torch.cuda.synchronize()
        # the window's rows, copied off the device, are the reference's input (and the twin's rows)
        rows = np.zeros(len(want), dtype=replay.EDGE_OUT_DTYPE)
        assert hip.hipMemcpy(rows.ctypes.data, ctypes.c_void_p(ptr), rows.nbytes, 2) == 0
        assert rows.tobytes() == want.tobytes() and len(rows) > 1000
        sel = ref_select(rows, k, ms)
        n_sel = int(d_n.item())
        assert n_sel == len(sel) > 0
        m = min(n_sel, cap)
        assert np.array_equal(d_idx.cpu().numpy()[:m].astype(np.uint32), sel[:m])
        assert d_out.cpu().numpy()[: m * 64].tobytes() == rows[sel[:m]].tobytes()


def test_histogram_engine_selected_rows_and_bins(trace):
    topo, ev, labels = trace
    a, b = _twins(topo, labels, 2, variant=2, max_window_events=300_000, max_batch=1 << 14, edge_histogram=True)
    w = ev[:150_000]
    _feed(a, w); _feed(b, w)
    rows, idx, n = a.flush_window_top(1000, NEG_INF)
    want = b.flush_window()
    _check(rows, idx, n, want, 1000, NEG_INF)
    assert np.array_equal(rows["p50_us"], want["p50_us"][idx]) and np.array_equal(rows["p99_us"], want["p99_us"][idx])
    assert want["p99_us"].any()
    assert np.array_equal(a.window_hist()[idx], b.window_hist()[idx])


def test_config3_full_size_top_k_and_threshold():
    topo = replay.make_topology(10_000, 1_000_000, replay.SEED_BASE + 3)
    ev, labels = replay.make_events(topo, 10_000_000, replay.SEED_BASE + 3)
    kw = dict(max_labels=128, max_outbound_ips=128, max_window_events=len(ev))
    a = _engine(topo.n_nodes, 1_250_000, 2, **kw); b = _engine(topo.n_nodes, 1_250_000, 2, **kw)
    for g in (a, b):
        HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    _feed(a, ev); _feed(b, ev)
    rows, idx, n = a.flush_window_top(1000, NEG_INF)
    want = b.flush_window().copy()
    assert n == len(want) > 1_000_000
    _check(rows, idx, n, want, 1000, NEG_INF)
    t = float(np.quantile(want["score"], 0.99))
    _feed(a, ev); _feed(b, ev)
    rows, idx, n = a.flush_window_top(0, t, cap=len(want))
    want = b.flush_window()
    _check(rows, idx, n, want, 0, t)
    assert len(rows) > 1000


def test_graphds_sink_receives_the_twins_top_k_in_selection_order():
    from alaz_amd import hostlib
    topo = replay.make_topology(200, 4000, seed=95)
    ev, labels = replay.make_events(topo, 60_000, seed=96, mixed=True)
    wire = replay.to_wire(ev, labels)
    W = weights.make_weights(2)
    gs = []
    for _ in range(2):
        cfg = engine.make_config(max_known_nodes=topo.n_nodes + 8, max_edges=8192, layers=2, max_outbound_ips=256, max_window_events=1 << 17)
        g = hostlib.GraphDS(cfg, batch=1000)
        g.set_clock(*CLOCK); g.load_weights(W); g.apply_ops(topo.k8s_ops())
        gs.append(g)
    a, b = gs
    assert a.set_selection(50, NEG_INF) == 0
    assert a.ingest_wire(wire) == 0 and b.ingest_wire(wire) == 0
    na, got = a.FlushWindowRows(10)
    nb, full = b.FlushWindowRows(10)
    assert na == nb == len(full) > 50
    score = np.array([r[9] for r in full], dtype=np.float32)
    order = np.lexsort((np.arange(len(full)), -(score.astype(np.float64) + 0.0)))[:50]
    assert got == [full[i] for i in order]
