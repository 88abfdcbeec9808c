"""The two forms of k5_edge_score (alaz_amd/csrc/sg_k5.h) on the development build: SG_K5_FORM=0 gives sixteen lanes to an edge, =1 one
lane (k5_edge_score_lanes: a wave takes 64 consecutive CSR positions per batch, P and Q rows pass through LDS, the weights through
scalar registers); geometry()["k5_form"] confirms which one ran.

Every case runs the same windows through one engine per form.  The rows (ordered by (from_ref, to_ref)) must be equal BYTE FOR BYTE
— the score's rounding points included — and the statistics counters equal; form 1 is also held to the oracle.  Shapes: nothing to
score, one edge, a batch boundary (63 / 64 / 65), more waves than batches (every small window: the grid follows max_edges), the mixed
36 000-edge trace of test_gpu_pair_tiles (all three ref kinds, alive records) with one layer and two, through the one-call pipeline
with its fused reset and through the staged calls, the histogram engine's percentiles, a window beyond max_edges, and a hub row beside
one-edge rows."""
import os

import numpy as np
import pytest

from alaz_amd import weights
from tests.gpu_model_scaffold import MAX_LABELS, STATS, _check_oracle, _close, _feed, _mixed, _on_edges, _oracle_windows, _sorted, _topo
from tests.helpers import CLOCK, HostShim

pytestmark = pytest.mark.gpu


def _engine(form, layers=1, max_edges=65536, **kw):
    from alaz_amd import engine
    topo, ops, _, _, labels = _topo()
    os.environ["SG_K5_FORM"] = str(form)
    try:
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=MAX_LABELS, max_outbound_ips=512,
                                max_window_events=1 << 18, dev_knobs=True, **{"k1_variant": 3, **kw})
    finally:
        os.environ.pop("SG_K5_FORM", None)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(layers))
    shim = HostShim(); shim.apply(g, ops)
    g.set_label_count(len(labels))
    assert g.geometry()["k5_form"] == form
    return g, shim


def _windows(form, windows, how="flush", layers=1, **kw):
    """one engine of this form over the windows: per window (sorted rows, counters, the window's outbound IPs), then the shim"""
    g, shim = _engine(form, layers, **kw)
    out = []
    for ev in windows:
        _feed(g, ev)
        rows = _sorted(_close(g, how, layers))
        st = g.stats()
        out.append((rows, {k: int(getattr(st, k)) for k in STATS}, g.outbound_ips().copy()))
    g.close()
    return out, shim


def _both(windows, **kw):
    """both forms over the same windows: equal rows, byte for byte, and equal counters.  Returns form 1's."""
    a, shim = _windows(1, windows, **kw)
    b, _ = _windows(0, windows, **kw)
    for i, ((ra, sa, oa), (rb, sb, ob)) in enumerate(zip(a, b)):
        assert sa == sb and np.array_equal(oa, ob), (i, sa, sb)
        assert len(ra) == len(rb), (i, len(ra), len(rb))
        if ra.tobytes() != rb.tobytes():
            bad = [n for n in ra.dtype.names if not np.array_equal(ra[n], rb[n])]
            d = np.flatnonzero(ra["score"].view(np.uint32) != rb["score"].view(np.uint32))
            raise AssertionError(f"window {i}: form 1's rows differ from form 0's in {bad}; {len(d)} of {len(ra)} scores, first {ra['score'][d[:3]]} vs {rb['score'][d[:3]]}")
    return a, shim


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_small_windows_and_batch_boundaries(n):
    """n distinct edges, one request each: no batch at all, one lane of one batch, one lane short of a batch, a whole batch, a second batch
    of one row, and sixteen batches (the last of 40 rows) for the 1 024 waves of the grid"""
    ev = _on_edges(np.arange(n), np.random.default_rng(500 + n))
    res, shim = _both([ev])
    assert len(res[0][0]) == n and res[0][1]["last_window_edges"] == n
    if n:
        _check_oracle(res, shim, _oracle_windows(("small", n), [ev], 1))


@pytest.mark.parametrize("layers", [1, 2])
def test_the_mixed_trace_through_flush_window(layers):
    ev = _mixed()
    res, shim = _both([ev], layers=layers)
    assert len(res[0][0]) > 20_000
    assert len(np.unique(res[0][0]["from_ref"] >> 30)) > 1 or len(np.unique(res[0][0]["to_ref"] >> 30)) > 1   # more than one ref kind
    assert int(res[0][0]["alive"].sum()) > 0
    _check_oracle(res, shim, _oracle_windows(("mixed", layers), [ev], layers))


def test_window_run_twice_the_fused_reset_ran():
    """sg_window_run folds the window reset into the score kernel: a second window through the same engine is right only if it ran"""
    wins = [_mixed(), _mixed(65536, 65536 + 40_000)]
    res, shim = _both(wins, how="run")
    _check_oracle(res, shim, _oracle_windows(("run2",), wins, 1))


def test_the_staged_calls():
    ev = _mixed()
    res, shim = _both([ev], how="staged", layers=2)
    _check_oracle(res, shim, _oracle_windows(("mixed", 2), [ev], 2))


def test_histogram_engine_percentiles():
    """k1_variant=2 with edge_histogram keeps a latency histogram per edge: p50_us / p99_us come off it, once per lane in form 1"""
    rng = np.random.default_rng(61)
    e = rng.integers(0, 3000, 40_000); e[:3000] = np.arange(3000)
    ev = _on_edges(e, rng)
    a, _ = _windows(1, [ev], k1_variant=2, edge_histogram=True)
    b, _ = _windows(0, [ev], k1_variant=2, edge_histogram=True)
    ra, rb = a[0][0], b[0][0]
    assert len(ra) == len(rb) == 3000 and a[0][1] == b[0][1]
    assert np.array_equal(ra["p50_us"], rb["p50_us"]) and np.array_equal(ra["p99_us"], rb["p99_us"])
    assert int(ra["p99_us"].max()) > 0 and bool((ra["p50_us"] <= ra["p99_us"]).all())
    assert ra.tobytes() == rb.tobytes()


def test_more_distinct_edges_than_max_edges():
    """4 096 rows at the most: both forms stop there.  (Which edges a full table keeps follows the order the workgroups reach it in; the
    rows are compared where both runs kept the same set.)"""
    ev = _on_edges(np.arange(6000), np.random.default_rng(62))
    a, _ = _windows(1, [ev], max_edges=4096)
    b, _ = _windows(0, [ev], max_edges=4096)
    ra, rb = a[0][0], b[0][0]
    assert len(ra) == len(rb) and 0 < len(ra) <= 4096
    assert a[0][1]["events_dropped_cap"] == b[0][1]["events_dropped_cap"] > 0
    for r in (ra, rb):
        key = (r["from_ref"].astype(np.uint64) << np.uint64(32)) | r["to_ref"]
        assert len(np.unique(key)) == len(r) and bool((r["count"] >= 1).all())
        assert bool(np.isfinite(r["score"]).all()) and bool(((r["score"] > 0) & (r["score"] < 1)).all())
    if np.array_equal(ra["from_ref"], rb["from_ref"]) and np.array_equal(ra["to_ref"], rb["to_ref"]):
        assert ra.tobytes() == rb.tobytes()


def test_a_hub_row_beside_one_edge_rows():
    """pod 5 calls 150 destinations (a row of more than two batches: every lane of a wave gathers the same P row), then 200 pods call one
    destination each (all sources different within a wave), then the hub again"""
    topo, _, _, plain, _ = _topo()
    rng = np.random.default_rng(63)
    dst = np.arange(10, 160)
    src = np.concatenate([np.full(150, 5), np.arange(200, 400), np.full(150, 5)])
    to = np.concatenate([dst, np.arange(600, 800), dst])
    ev = np.repeat(plain[:1], len(src))
    ev["flags"] = 0; ev["host_label"] = 0
    ev["saddr"] = topo.pod_ips[src]; ev["daddr"] = topo.pod_ips[to]
    ev["duration_ns"] = rng.integers(1, 1 << 30, len(src)); ev["status"] = 200
    res, shim = _both([ev])
    rows = res[0][0]
    assert len(rows) == 350 and int(np.bincount(rows["from_ref"] & 0x3FFFFFFF).max()) == 150
    _check_oracle(res, shim, _oracle_windows(("hub",), [ev], 1))
