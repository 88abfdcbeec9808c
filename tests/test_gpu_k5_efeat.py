"""The edge features inside the score kernel (alaz_amd/csrc/sg_k5.h: k5_edge_score_lanes<RESET, EFEAT = true>) on the development
build: with SG_K5_EFEAT=1 a lane of form 1 computes e_uv, lat_z and err_ratio of its own edge from the accumulators it loads anyway
(edge_feature_values, sg_k2.h — the one copy of the arithmetic), k3_node_features launches no edge workgroups and the engine holds no
efeat / latz / errr arrays; with =0 those workgroups store the values and the score kernel loads them.  geometry()["k5_efeat"]
confirms which one ran.

Every case runs the same windows through twin engines of form 1, one per setting.  The rows (ordered by (from_ref, to_ref)) must be
equal BYTE FOR BYTE — the features' roundings included: the score kernel sits under `fp contract(off)`, the feature code does not —
and the statistics counters equal; the inline engine is also held to the oracle.  Shapes: the batch boundaries of form 1, the mixed
36 000-edge trace through all three ways to close a window, and one case per arm of edge_feature_values: no requests on an edge
(rc = 0), the ends of the log1p table (4095 / 4096 / 4097 requests, and as many errors), a row of one edge (sd = 0) beside a hub row
(sd > 1), equal durations (var <= 0), lat_z clamped on both sides for the feature, the histogram engine, a full edge table and two
windows in flight.

Not covered here: the `cnt | err >= 2^24` arm of err_ratio needs 16.7 M requests on one edge, which is no few-second case; it is left to
the C3 comparison of all 14 `bench.py --dump-outputs` files against the parent commit (profiles/k5_efeat_ab_c3.txt) — whose 10 M-event
window does not reach it either: the arm is one source expression for both forms and has not run in this comparison."""
import ctypes
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.gpu_model_scaffold import MAX_LABELS, STATS, _check_oracle, _close, _feed, _mixed, _on_edges, _oracle_windows, _sorted, _topo
from tests.helpers import CLOCK, HostShim

pytestmark = pytest.mark.gpu


def _engine(efeat, layers=1, max_edges=65536, **kw):
    from alaz_amd import engine
    topo, ops, _, _, labels = _topo()
    os.environ["SG_K5_FORM"] = "1"; os.environ["SG_K5_EFEAT"] = str(efeat)
    try:
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=MAX_LABELS, max_outbound_ips=512,
                                max_window_events=1 << 18, dev_knobs=True, **{"k1_variant": 3, **kw})
    finally:
        os.environ.pop("SG_K5_FORM", None); os.environ.pop("SG_K5_EFEAT", None)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(layers))
    shim = HostShim(); shim.apply(g, ops)
    g.set_label_count(len(labels))
    geo = g.geometry()
    assert geo["k5_form"] == 1 and geo["k5_efeat"] == efeat
    return g, shim


def _windows(efeat, windows, how="flush", layers=1, **kw):
    """one engine over the windows: per window (sorted rows, counters, the window's outbound IPs), then the shim"""
    g, shim = _engine(efeat, layers, **kw)
    out = []
    for ev in windows:
        _feed(g, ev)
        rows = _sorted(_close(g, how, layers))
        st = g.stats()
        out.append((rows, {k: int(getattr(st, k)) for k in STATS}, g.outbound_ips().copy()))
    g.close()
    return out, shim


def _same_rows(i, ra, rb):
    assert len(ra) == len(rb), (i, len(ra), len(rb))
    if ra.tobytes() != rb.tobytes():
        bad = [n for n in ra.dtype.names if not np.array_equal(ra[n].view(np.uint8), rb[n].view(np.uint8))]
        d = np.flatnonzero((ra["score"].view(np.uint32) != rb["score"].view(np.uint32)) | (ra["lat_z"].view(np.uint32) != rb["lat_z"].view(np.uint32)) |
                           (ra["err_ratio"].view(np.uint32) != rb["err_ratio"].view(np.uint32)))
        raise AssertionError(f"window {i}: the inline features' rows differ from the stored features' in {bad}; {len(d)} of {len(ra)} rows, first "
                             f"{ra[['count', 'err_count', 'score', 'lat_z', 'err_ratio']][d[:3]]} vs {rb[['count', 'err_count', 'score', 'lat_z', 'err_ratio']][d[:3]]}")


def _both(windows, **kw):
    """the twin engines over the same windows: equal rows, byte for byte, and equal counters.  Returns the inline engine's."""
    a, shim = _windows(1, windows, **kw)
    b, _ = _windows(0, windows, **kw)
    for i, ((ra, sa, oa), (rb, sb, ob)) in enumerate(zip(a, b)):
        assert sa == sb and np.array_equal(oa, ob), (i, sa, sb)
        _same_rows(i, ra, rb)
    return a, shim


def _pods(src, to, dur, status=200):
    """one plain request per entry, pod src[i] -> pod to[i]"""
    topo, _, _, plain, _ = _topo()
    ev = np.repeat(plain[:1], len(src))
    ev["flags"] = 0; ev["host_label"] = 0
    ev["saddr"] = topo.pod_ips[np.asarray(src)]; ev["daddr"] = topo.pod_ips[np.asarray(to)]
    ev["duration_ns"] = dur; ev["status"] = status
    return ev


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_small_windows_and_batch_boundaries(n):
    """n distinct edges, one request each (every one a row of its own statistics or a short one): no batch, one lane, a lane short of a
    batch, a whole batch, a second batch of one row — whose next-batch loads are the clamped ones —, sixteen batches"""
    ev = _on_edges(np.arange(n), np.random.default_rng(500 + n))
    res, shim = _both([ev])
    assert len(res[0][0]) == n and res[0][1]["last_window_edges"] == n
    if n:
        _check_oracle(res, shim, _oracle_windows(("small", n), [ev], 1))


@pytest.mark.parametrize("layers", [1, 2])
def test_the_mixed_trace_through_flush_window(layers):
    ev = _mixed()
    res, shim = _both([ev], layers=layers)
    assert len(res[0][0]) > 20_000 and int(res[0][0]["alive"].sum()) > 0
    _check_oracle(res, shim, _oracle_windows(("mixed", layers), [ev], layers))


def test_window_run_twice_the_fused_reset_ran():
    """the one-call pipeline (k5_edge_score_lanes<true, .>): the second window is right only if the first one's reset ran"""
    wins = [_mixed(), _mixed(65536, 65536 + 40_000)]
    res, shim = _both(wins, how="run")
    _check_oracle(res, shim, _oracle_windows(("run2",), wins, 1))


def test_the_staged_calls():
    """sg_window_features launches the node workgroups alone, sg_window_score the kernel without the reset"""
    ev = _mixed()
    res, shim = _both([ev], how="staged", layers=2)
    _check_oracle(res, shim, _oracle_windows(("mixed", 2), [ev], 2))


def test_an_edge_of_open_connections_only():
    """edges 100..199 see open-connection records and no request: count = 0, so rc = 0, the mean and err_ratio 0, log1p(0) off the table"""
    rng = np.random.default_rng(71)
    ev = _on_edges(np.arange(200), rng)
    topo = _topo()[0]
    ev["flags"][100:] = replay.EV_ALIVE
    ev["saddr"][100:] = topo.pod_ips[topo.edge_src[np.arange(100, 200)]]
    res, shim = _both([ev])
    rows = res[0][0]
    idle = rows[rows["count"] == 0]
    assert len(idle) > 0 and bool((idle["alive"] > 0).all()) and bool((idle["err_ratio"] == 0).all())
    _check_oracle(res, shim, _oracle_windows(("alive-only",), [ev], 1))


def test_the_ends_of_the_log1p_table():
    """the table holds log1p of 0 .. 4095: requests and errors of 4095, 4096 and 4097 on an edge take its last entry and the fp64 log1p
    beyond it; three more edges carry the same requests without an error"""
    rng = np.random.default_rng(72)
    counts = [4095, 4096, 4097]
    e = np.concatenate([np.full(c, i) for i, c in enumerate(counts)] + [np.full(c, 3 + i) for i, c in enumerate(counts)])
    ev = _on_edges(e, rng)
    ev["status"] = np.where(e < 3, 503, 200)
    res, shim = _both([ev])
    rows = res[0][0]
    assert sorted(rows["count"].tolist()) == sorted(counts * 2)
    assert sorted(rows["err_count"].tolist()) == [0, 0, 0] + counts
    _check_oracle(res, shim, _oracle_windows(("l1p-ends",), [ev], 1))


def test_a_hub_row_beside_one_edge_rows():
    """pod 5 calls 150 destinations with durations up to a second (its row: sd > 1, lat_z divided by it), 200 pods call one destination
    each (a row of one edge: sd = 0, lat_z = m_e - mu, zero but for the last bit of the two means)"""
    rng = np.random.default_rng(63)
    dst = np.arange(10, 160)
    src = np.concatenate([np.full(150, 5), np.arange(200, 400), np.full(150, 5)])
    to = np.concatenate([dst, np.arange(600, 800), dst])
    ev = _pods(src, to, rng.integers(1, 1 << 30, len(src)))
    res, shim = _both([ev])
    rows = res[0][0]
    assert len(rows) == 350 and int(np.bincount(rows["from_ref"] & 0x3FFFFFFF).max()) == 150
    one = rows[rows["count"] == 1]
    assert len(one) == 200 and float(np.abs(one["lat_z"]).max()) < 1e-6   # (m_e - mu: the same quotient twice, to the last bits of 1e6 us in fp64)
    assert float(np.abs(rows[rows["count"] == 2]["lat_z"]).max()) > 0.5
    _check_oracle(res, shim, _oracle_windows(("efeat-hub",), [ev], 1))


def test_a_row_of_equal_durations():
    """pod 7 calls 40 destinations five times each, every request 3 000 000 ns: the mean square equals the square of the mean on every
    edge and in the row — var <= 0 takes s_e = 0, the row's sd <= 1 takes lat_z = m_e - mu, zero but for the last bit of the two means"""
    src = np.full(200, 7)
    to = np.tile(np.arange(300, 340), 5)
    ev = _pods(src, to, 3_000_000)
    res, shim = _both([ev])
    rows = res[0][0]
    assert len(rows) == 40 and bool((rows["count"] == 5).all()) and float(np.abs(rows["lat_z"]).max()) < 1e-6
    _check_oracle(res, shim, _oracle_windows(("equal",), [ev], 1))


def test_lat_z_beyond_eight_on_both_sides():
    """one slow edge among 149 fast ones of pod 5 (lat_z ~ +12), one fast edge among 149 slow ones of pod 6 (~ -12): the row keeps
    lat_z, the feature is clamped at +-8"""
    rng = np.random.default_rng(74)
    dst = np.arange(10, 160)
    hi = rng.integers(1_000_000, 1_001_000, 150); hi[17] = 1 << 30
    lo = rng.integers((1 << 30) - 1000, 1 << 30, 150); lo[23] = 1000
    ev = _pods(np.concatenate([np.full(150, 5), np.full(150, 6)]), np.concatenate([dst, dst]), np.concatenate([hi, lo]))
    res, shim = _both([ev])
    rows = res[0][0]
    assert len(rows) == 300 and float(rows["lat_z"].max()) > 8 and float(rows["lat_z"].min()) < -8
    _check_oracle(res, shim, _oracle_windows(("latz",), [ev], 1))


def test_more_distinct_edges_than_max_edges():
    """4 096 rows at the most.  (Which edges a full table keeps follows the order the workgroups reach it in; the rows are compared
    where both runs kept the same set.)"""
    ev = _on_edges(np.arange(6000), np.random.default_rng(62))
    a, _ = _windows(1, [ev], max_edges=4096)
    b, _ = _windows(0, [ev], max_edges=4096)
    ra, rb = a[0][0], b[0][0]
    assert len(ra) == len(rb) and 0 < len(ra) <= 4096
    assert a[0][1]["events_dropped_cap"] == b[0][1]["events_dropped_cap"] > 0
    key = (ra["from_ref"].astype(np.uint64) << np.uint64(32)) | ra["to_ref"]
    assert len(np.unique(key)) == len(ra) and bool((ra["count"] >= 1).all())
    assert bool(np.isfinite(ra["score"]).all()) and bool(((ra["score"] > 0) & (ra["score"] < 1)).all())
    if np.array_equal(ra["from_ref"], rb["from_ref"]) and np.array_equal(ra["to_ref"], rb["to_ref"]):
        _same_rows(0, ra, rb)


def test_histogram_engine_percentiles():
    """k1_variant=2 with edge_histogram: the percentiles take the accumulators the lane reloads for its row, not the feature block's"""
    rng = np.random.default_rng(61)
    e = rng.integers(0, 3000, 40_000); e[:3000] = np.arange(3000)
    ev = _on_edges(e, rng)
    a, _ = _windows(1, [ev], k1_variant=2, edge_histogram=True)
    b, _ = _windows(0, [ev], k1_variant=2, edge_histogram=True)
    ra, rb = a[0][0], b[0][0]
    assert len(ra) == len(rb) == 3000 and a[0][1] == b[0][1]
    assert int(ra["p99_us"].max()) > 0 and bool((ra["p50_us"] <= ra["p99_us"]).all())
    _same_rows(0, ra, rb)


def test_two_windows_in_flight():
    """windows_in_flight = 2: two windows closed back to back on their own slots and streams — every slot without feature arrays —
    give the rows of the one-slot engine that stores the features"""
    import torch
    wins = [_mixed(0, 40_000), _mixed(65536, 65536 + 40_000)]
    want, _ = _windows(0, wins)
    g, _ = _engine(1, windows_in_flight=2)
    try:
        hip = g._l                                                   # (the engine's library: dlsym on its handle reaches the HIP runtime it is linked against)
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]; hip.hipMemcpy.restype = ctypes.c_int
        dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in wins]
        torch.cuda.synchronize()
        ptrs = []
        for i, w in enumerate(wins):
            g.ingest_device(dev[i].data_ptr(), len(w), 0)
            g.window_run(0)
            ptrs.append(g.rows_buffer())
        torch.cuda.synchronize()
        assert len(set(ptrs)) == 2
        for i, p in enumerate(ptrs):
            buf = np.zeros(len(want[i][0]), dtype=replay.EDGE_OUT_DTYPE)
            assert len(buf) and hip.hipMemcpy(buf.ctypes.data, ctypes.c_void_p(p), len(buf) * 64, 2) == 0
            _same_rows(i, _sorted(buf), want[i][0])
    finally:
        g.close()
