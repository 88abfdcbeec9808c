"""K3's two batched-load forms on the development build (alaz_amd/csrc/sg_k3.h): SG_K3_IN_FORM=1 runs k3_in_part<1> (every load of a
trip unconditional and issued together; a lane outside the range loads the slice's first position and drops it), SG_K3_FEAT_LANES=1
runs k3_node_features_lanes (eight lanes per node: the partials in one batch, a butterfly, two chains per lane, one float4 per lane).
geometry()["k3_in_form"] / ["k3_feat_lanes"] confirm which ran.

Every case runs the same windows through four twin engines — (in_form, feat_lanes) = (0, 0), (1, 0), (0, 1), (1, 1), all of K5's form 1
with the edge features inline, which the eight-lane kernel needs — and holds the last three to the first BYTE FOR BYTE: st_sum / st_max
(where a pipeline stops before the reset), x0 and every h[l] over the whole capacity (filled with NaN before each window, so a row
written past N or left unwritten below it shows), the rows, the node rows where the rollup is on (they carry the in-statistics of the
one-call pipelines, whose st_sum the reset clears) and the sg_stats counters.  The (1, 1) engine is also held to the oracle, or to
model_ref's references of its own rows where the oracle is not closed at that size.

Shapes (the slice count comes from SG_K3_SLICES, so that a slice is small):
  scan      0 and 1 edges; one slice of exactly 8 192 and of 8 193 positions (a second trip of one edge, its prefetch clamped); slice
            lengths that are no multiple of 1 024; more slices than edges (empty slices); a last slice shorter than the others; the
            boundary trace (in-edges at nodes 3 071 / 3 072, 6 143 / 6 144: the range boundaries; at 48 and 70 slices most slices hold
            no edge into the third range, so every lane takes the shared address); 64 consecutive positions with one destination; edges
            with and without errors; an edge of open connections only; more distinct edges than max_edges
  features  1, 7, 8, 9, 31, 32 and 33 nodes; 3, 8, 9, 48 and 70 slices; the staged calls (S_in = 0 behind k3_in_reduce); nodes without
            in-edges, without out-edges, label and raw-IP nodes (kind 0); maxima of 2^32 ns and more; a node capacity one past the
            grid cap of 2 048 workgroups x 32 nodes
  pipelines flush_window, window_run twice, a warm engine over a cold, a warm and a delta window (kw_finish_rows rides in k3_in_part's
            launch), two windows in flight"""
import ctypes

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.gpu_model_scaffold import C_COUNT, C_N_NODES, MAX_LABELS, STATS, _check_oracle, _feed, _mixed, _on_edges, _oracle_windows, _sorted, _topo, bits, check_rows, check_stats, check_x0, dev_read, dev_write, knobs, oracle, trace
from tests.helpers import CLOCK, HostShim
from tests import model_ref as mr

pytestmark = pytest.mark.gpu

SETTINGS = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.fixture(scope="module", autouse=True)
def _hip_symbols():
    """dev_read / dev_write of test_gpu_model_stages look hipMemcpy up among the process's global symbols: the shipped library is the
    one loaded globally (the development build, which every engine here runs, is loaded locally)"""
    from alaz_amd import engine
    engine.load_library()


class Twin:
    """one engine of a setting with its buffers; window() runs one window and returns everything that is compared"""

    def __init__(self, setting, make, layers, slices=None, nodes=False):
        kv = dict(SG_K5_FORM=1, SG_K5_EFEAT=1, SG_K3_IN_FORM=setting[0], SG_K3_FEAT_LANES=setting[1])
        if slices is not None:
            kv["SG_K3_SLICES"] = slices
        with knobs(**kv):
            self.g, self.shim = make()
        self.layers, self.nodes = layers, nodes
        geo = self.g.geometry()
        assert (geo["k5_form"], geo["k5_efeat"], geo["k3_in_form"], geo["k3_feat_lanes"]) == (1, 1) + tuple(setting), geo
        if nodes:
            self.g.set_nodes(True)

    def buffers(self):
        s, m, c, ncap = self.g.window_buffers()
        return s, m, c, ncap, [self.g.feat_buffer(l) for l in range(self.layers + 1)]

    def read_stats(self, out, tag):
        s, m, c, ncap, _ = self.buffers()
        out[f"st_sum {tag}"] = dev_read(s, (ncap, mr.SUM_WORDS), np.uint64)
        out[f"st_max {tag}"] = dev_read(m, (ncap, mr.MAX_WORDS), np.uint64)
        out["n"] = int(dev_read(c, (C_COUNT,), np.uint64)[C_N_NODES])

    def window(self, ev, how):
        g, L, out = self.g, self.layers, {}
        _, _, _, ncap, feat = self.buffers()
        for p, w in feat:
            dev_write(p, np.full((ncap, w), np.nan, dtype=np.float32))
        _feed(g, ev)
        if how == "staged":
            g.window_close(); self.read_stats(out, "after the close")
            g.window_features(); self.read_stats(out, "after the features")
            for l in range(L):
                g.window_layer(l)
            g.window_score()
            rows = g.window_read().copy()
            g.window_reset()
        elif how == "run":
            g.window_run()
            rows = g.window_read().copy()
        else:
            rows = g.flush_window().copy()
        if self.nodes:
            out["node rows"] = g.window_nodes().copy()
        _, _, _, ncap, feat = self.buffers()
        for l, (p, w) in enumerate(feat):
            out["x0" if l == 0 else f"h[{l}]"] = dev_read(p, (ncap, w), np.float32)
        out["rows"] = _sorted(rows)
        out["_in order"] = rows                                      # (not compared: a full table keeps its edges in the order the workgroups reached it)
        st = g.stats()
        out["stats"] = {k: int(getattr(st, k)) for k in STATS}
        out["ob"] = g.outbound_ips().copy()
        return out

    def close(self):
        self.g.close()


def same(tag, a, b, skip=()):
    assert sorted(a) == sorted(b), (tag, sorted(a), sorted(b))
    for k in a:
        if k in skip or k.startswith("_"):
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (tag, k, a[k].shape, b[k].shape)
            if a[k].tobytes() != b[k].tobytes():
                av, bv = (x.reshape(len(x), -1).view(np.uint8) if len(x) else x for x in (a[k], b[k]))
                bad = np.flatnonzero((av != bv).any(axis=1))
                raise AssertionError(f"{tag}: {k} differs from the (0, 0) engine's in {len(bad)} of {len(av)} rows, first {bad[:6].tolist()}: "
                                     f"{a[k][bad[0]]} vs {b[k][bad[0]]}")
        else:
            assert a[k] == b[k], (tag, k, a[k], b[k])


def twins(make, windows, how="flush", layers=1, slices=None, nodes=False, skip=(), settings=SETTINGS):
    """the windows through one engine per setting; every setting held to (0, 0).  -> the (1, 1) engine's windows and its shim"""
    res = {}
    for st in settings:
        t = Twin(st, make, layers, slices, nodes)
        try:
            res[st] = [t.window(ev, how) for ev in windows], t.shim
        finally:
            t.close()
    for st in settings[1:]:
        for i, (a, b) in enumerate(zip(res[st][0], res[settings[0]][0])):
            same(f"setting {st}, window {i} ({how})", a, b, skip)
    return res[settings[-1]]


def topo_engine(layers=1, max_edges=65536, **kw):
    """the 2 000-pod topology of test_gpu_pair_tiles (with labels and raw outbound IPs in its mixed trace)"""
    def make():
        from alaz_amd import engine
        topo, ops, _, _, labels = _topo()
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=MAX_LABELS, max_outbound_ips=512,
                                max_window_events=1 << 18, dev_knobs=True, **{"k1_variant": 3, **kw})
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(layers))
        shim = HostShim(); shim.apply(g, ops)
        g.set_label_count(len(labels))
        return g, shim
    return make


def trace_engine(name, layers, max_edges=32768, **kw):
    """an engine on a trace of test_gpu_model_stages, as its Eng builds one"""
    def make():
        from alaz_amd import engine
        topo, ev, labels = trace(name)
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, layers=layers, max_labels=128, max_outbound_ips=512, k1_variant=3,
                                max_window_events=len(ev) + 1, max_edges=max_edges, dev_knobs=True, **kw)
        g.set_clock(*CLOCK)
        shim = HostShim(); shim.apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
        g.load_weights(weights.make_weights(layers))
        return g, shim
    return make


def check_topo_oracle(res, key, windows, layers=1):
    got, shim = res
    _check_oracle([(w["rows"], w["stats"], w["ob"]) for w in got], shim, _oracle_windows(("k3forms",) + key, windows, layers))


def check_trace_oracle(w, name, layers, tag, staged=False):
    """one window of the (1, 1) engine on a model_stages trace: rows, x0 (1 ulp of the oracle and of the float64 reference, zeros and
    the constant column in place), and after the staged features the statistics, word for word"""
    o = oracle(name, layers)
    N = o["n"]
    check_rows(w["_in order"], o["rows"], tag)
    assert np.isnan(w["x0"][N:]).all(), (tag, "x0 written beyond the window's nodes")
    check_x0(w["x0"][:N], o, tag)
    if staged:
        class E:                                                     # (what check_stats asks of an engine)
            def n_nodes(self): return w["n"]
            def stats(self): return w["st_sum after the features"], w["st_max after the features"]
        check_stats(E(), o, tag)


def pods(src, to, dur, status=200):
    """one plain request per entry, pod src[i] -> pod to[i] of the 2 000-pod topology"""
    topo, _, _, plain, _ = _topo()
    ev = np.repeat(plain[:1], len(src))
    ev["flags"] = 0; ev["host_label"] = 0
    ev["saddr"] = topo.pod_ips[np.asarray(src)]; ev["daddr"] = topo.pod_ips[np.asarray(to)]
    ev["duration_ns"] = dur; ev["status"] = status
    return ev


# ------------------------------------------------------------------------------------------------
# the scan
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slices", [(0, 1), (1, 1), (1, 3), (5, 8), (1000, 1), (1000, 3), (8192, 1), (8193, 1), (8193, 3), (20000, 2)])
def test_scan_trips_slices_and_their_ends(n, slices):
    """n distinct edges, one request each (one in ten an error), in `slices` slices of ceil(n / slices) positions: nothing to scan; one
    lane; empty slices (1 edge in 3 slices, 5 in 8); lengths that are no multiple of 1 024, with a shorter last slice (1 000 in 3:
    334 + 334 + 332); exactly one trip (8 192) and a second trip of ONE edge (8 193), whose eight prefetches are all clamped but the
    first; 8 193 in 3 and 20 000 in 2 (two trips, the second partly past the end)"""
    ev = _on_edges(np.arange(n), np.random.default_rng(900 + n))
    res = twins(topo_engine(), [ev], slices=slices)
    w = res[0][0]
    assert len(w["rows"]) == n and w["stats"]["last_window_edges"] == n
    if n:
        assert n < 100 or int((w["rows"]["err_count"] > 0).sum()) > 0
        check_topo_oracle(res, ("distinct", n), [ev])


def test_sixty_four_consecutive_positions_with_one_destination():
    """pods 100 .. 163 call pod 5 and nothing else (64 consecutive CSR positions, one wave's worth of LDS atomics on one node), pods
    300 .. 363 call pod 5 and pod 6 (the same destination at every second position); staged, so that st_sum is read"""
    src = np.concatenate([np.arange(100, 164), np.arange(300, 364), np.arange(300, 364)])
    to = np.concatenate([np.full(128, 5), np.full(64, 6)])
    ev = pods(src, to, np.random.default_rng(64).integers(1, 1 << 30, len(src)))
    for how in ("staged", "flush"):
        res = twins(topo_engine(), [ev], how=how, slices=2)
        assert len(res[0][0]["rows"]) == 192
    check_topo_oracle(res, ("one-dst",), [ev])


def test_an_edge_of_open_connections_only():
    """edges 100 .. 199 see open-connection records and no request: accumulators of zero under a degree of one"""
    ev = _on_edges(np.arange(200), np.random.default_rng(71))
    topo = _topo()[0]
    ev["flags"][100:] = replay.EV_ALIVE
    ev["saddr"][100:] = topo.pod_ips[topo.edge_src[np.arange(100, 200)]]
    res = twins(topo_engine(), [ev], slices=3)
    rows = res[0][0]["rows"]
    idle = rows[rows["count"] == 0]
    assert len(idle) > 0 and bool((idle["alive"] > 0).all())
    check_topo_oracle(res, ("alive-only",), [ev])


def test_more_distinct_edges_than_max_edges():
    """4 096 rows at the most.  (Which edges a full table keeps follows the order the workgroups reach it in; the twins are compared
    where they kept the same set.)"""
    ev = _on_edges(np.arange(6000), np.random.default_rng(62))
    got = {}
    for st in SETTINGS:
        t = Twin(st, topo_engine(max_edges=4096), 1, 3)
        try:
            got[st] = t.window(ev, "flush")
        finally:
            t.close()
    a = got[(0, 0)]
    assert 0 < len(a["rows"]) <= 4096 and a["stats"]["events_dropped_cap"] > 0
    for st in SETTINGS[1:]:
        b = got[st]
        assert len(b["rows"]) == len(a["rows"]) and b["stats"] == a["stats"]
        assert bool(np.isfinite(b["rows"]["score"]).all())
        if np.array_equal(a["rows"]["from_ref"], b["rows"]["from_ref"]) and np.array_equal(a["rows"]["to_ref"], b["rows"]["to_ref"]):
            same(f"setting {st}, a full table", b, a)


# ------------------------------------------------------------------------------------------------
# range boundaries, slice counts, the staged calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", [3, 8, 9, 48, 70])
def test_the_boundary_trace_at_slice_counts_on_both_sides_of_a_batch(slices):
    """model_ref.boundary_trace (three ranges; in-edges at 3 071 / 3 072 / 6 143 / 6 144 and N - 1; pod 3 071 has in-edges only, pod
    3 073 out-edges only; labels and raw IPs are kind 0) through flush_window — the eight-lane kernel sums the partials: fewer slices
    than lanes (3), one per lane (8), a second round of one (9), the plan's most (48: the 18-load batch full) and 70 (a 24-load batch
    and a second one, mostly clamped)"""
    res = twins(trace_engine("boundary", 2), [trace("boundary")[1]], layers=2, slices=slices, nodes=True)
    w = res[0][0]
    check_trace_oracle(w, "boundary", 2, f"boundary slices={slices}")
    assert len(w["node rows"]) > 6000


@pytest.mark.parametrize("name", ["boundary", "adversarial"])
def test_the_staged_calls(name):
    """sg_window_close launches k3_in_part without the finishing workgroups and k3_in_reduce behind it; sg_window_features the node
    launch with S_in = 0: both sides read st_sum.  The statistics after the close and after the features, word for word"""
    res = twins(trace_engine(name, 2, max_edges=32768), [trace(name)[1]], how="staged", layers=2, slices=5)
    check_trace_oracle(res[0][0], name, 2, f"{name} staged", staged=True)


def test_maxima_of_two_to_the_32_nanoseconds_and_more():
    """durations of 2^32 - 1, 2^32, 2^32 + 12 345 and 5 x 2^32 ns into pod 9 and out of pod 8: the maxima (and the sums) need their upper
    words through the butterfly"""
    dur = np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 12345, 5 << 32], dtype=np.uint64)
    ev = np.concatenate([pods([20, 21, 22, 23], [9, 9, 9, 9], dur), pods([8, 8, 8, 8], [30, 31, 32, 33], dur), pods(np.arange(40, 60), np.arange(60, 80), 1_000_000)])
    for how in ("staged", "flush"):
        res = twins(topo_engine(), [ev], how=how, slices=9, nodes=how == "flush")
    w = res[0][0]
    assert int(w["rows"]["max_ns"].max()) == 5 << 32
    for col in (8, 9):                                               # log1p(max / 1e6) of the out side and of the in side
        assert abs(float(np.nanmax(w["x0"][:, col])) - np.log1p((5 << 32) / 1e6)) < 1e-5
    check_topo_oracle(res, ("max32",), [ev])


def _tiny(n):
    """an engine with n pods and nothing else; every pod calls the next one, pod 0 also itself"""
    def make():
        from alaz_amd import engine
        g = engine.ServiceGraph(max_known_nodes=max(n, 8), max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, max_window_events=4096,
                                k1_variant=3, dev_knobs=True)
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(1))
        for i in range(n):
            g.upsert_pod(int(replay.POD_IP_BASE + i), i)
        return g, None
    ev = np.repeat(_topo()[3][:1], 3 * n + 1)
    ev["flags"] = 0; ev["host_label"] = 0; ev["status"] = 200
    src = np.concatenate([np.tile(np.arange(n), 3), [0]])
    ev["saddr"] = (replay.POD_IP_BASE + src).astype(np.uint32)
    ev["daddr"] = (replay.POD_IP_BASE + np.concatenate([(np.tile(np.arange(n), 3) + 1) % n, [0]])).astype(np.uint32)
    ev["duration_ns"] = np.random.default_rng(n).integers(1000, 1 << 28, len(ev))
    return make, ev


@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 32, 33])
def test_node_counts_around_a_wave_and_a_workgroup_of_the_eight_lane_kernel(n):
    """n nodes: one node in one wave (the other 31 groups of eight lanes idle on node 0's data), one short of a wave's eight nodes, a
    wave, one more, and the same around the workgroup's 32; x0 beyond row n stays NaN.  Held to node_features_ref of the engine's rows"""
    make, ev = _tiny(n)
    for how in ("staged", "flush"):
        got, _ = twins(make, [ev], how=how, slices=3)
    w = got[0]
    rows = w["rows"]
    assert len(rows) == (n + 1 if n > 1 else 1) and not (rows["from_ref"] >> 30).any()   # (the ring and pod 0 -> pod 0, which IS the ring at n = 1)
    N = int(max(rows["from_ref"].max(), rows["to_ref"].max())) + 1
    assert N == n and np.isnan(w["x0"][N:]).all() and np.isfinite(w["x0"][:N]).all()
    ref = mr.node_stats_ref(rows, N, rows["from_ref"].astype(np.int64), rows["to_ref"].astype(np.int64))
    d = mr.ulp_distance(w["x0"][:N], mr.node_features_ref(ref, np.full(N, mr.NODE_POD, dtype=np.uint8)))
    assert d.max() <= 1, np.argwhere(d > 1)[:4].tolist()


def test_a_node_capacity_one_workgroup_past_the_grid_cap():
    """65 700 pods: the eight-lane kernel's node loop (2 048 workgroups x 32 nodes) takes a second trip; in-edges and out-rows on both
    sides of node 65 536.  Held to node_stats_ref / node_features_ref of the engine's own rows (the oracle is not closed at this size)"""
    NP = 65_700
    topo, ev, _ = mr.sparse_trace(NP, NP - 150, 4000, seed=0x5A65, n_svcs=0)
    speak = np.unique(np.concatenate([ev["saddr"], ev["daddr"], topo.pod_ips[-1:]]).astype(np.int64) - replay.POD_IP_BASE)

    def make():
        from alaz_amd import engine
        g = engine.ServiceGraph(max_known_nodes=NP, max_edges=8192, layers=1, max_labels=16, max_outbound_ips=64, max_window_events=len(ev) + 1, dev_knobs=True)
        g.set_clock(*CLOCK)
        for i in speak:
            g.upsert_pod(int(topo.pod_ips[i]), int(i))
        g.load_weights(weights.make_weights(1))
        return g, None
    for how in ("staged", "flush"):
        got, _ = twins(make, [ev], how=how, slices=9, settings=[(0, 0), (1, 1)])
        w = got[0]
        rows = w["rows"]
        u, v = rows["from_ref"].astype(np.int64), rows["to_ref"].astype(np.int64)
        assert len(w["x0"]) > 65536 + 32 and (u >= 65536).sum() > 50 and (v >= 65536).sum() > 50 and (u < 65536).any() and (v < 65536).any()
        ref = mr.node_stats_ref(rows, NP, u, v)
        kind = np.zeros(NP, dtype=np.uint8); kind[speak] = mr.NODE_POD
        d = mr.ulp_distance(w["x0"][:NP], mr.node_features_ref(ref, kind))
        assert d.max() <= 1, (how, np.argwhere(d > 1)[:4].tolist())
        assert np.all(bits(w["x0"][:NP, 18:]) == 0) and np.all(w["x0"][:NP, 15] == 1.0) and np.isnan(w["x0"][NP:]).all()
        if how == "staged":
            assert w["n"] == NP and np.array_equal(w["st_sum after the features"][:NP], ref[0]) and np.array_equal(w["st_max after the features"][:NP], ref[1])


# ------------------------------------------------------------------------------------------------
# the pipelines
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2])
def test_the_mixed_trace_through_flush_window(layers):
    """36 000 edges of all three ref kinds with open connections, at the plan's own slice count; the node rows carry the in-statistics"""
    ev = _mixed()
    res = twins(topo_engine(layers), [ev], layers=layers, nodes=True)
    assert len(res[0][0]["rows"]) > 20_000 and int(res[0][0]["rows"]["alive"].sum()) > 0
    check_topo_oracle(res, ("mixed", layers), [ev], layers)


def test_window_run_twice():
    """the one-call pipeline with the fused reset: the second window's statistics start from what the first one's reset left, and the
    re-armed alive list"""
    wins = [_mixed(), _mixed(65536, 65536 + 40_000)]
    res = twins(topo_engine(), wins, how="run", slices=7)
    check_topo_oracle(res, ("run2",), wins)


def test_a_warm_engine_over_a_cold_a_warm_and_a_delta_window():
    """warm = True: the first window builds the kept state, the second closes warm (kw_finish_rows in the last workgroups of
    k3_in_part's launch writes the out-statistics the features read), the third brings edges the kept set does not hold (the
    C_KEPT_BUF flip by workgroup 0).  The boundary trace without raw outbound IPs, then every second event of it, then all of it"""
    ev = trace("boundary_known")[1]
    wins = [ev[::2].copy(), ev[::2].copy(), ev]
    warm = []

    def make():
        g, shim = trace_engine("boundary_known", 2, warm=True)()
        warm.append(g)
        return g, shim
    res = {}
    for st in SETTINGS:
        t = Twin(st, make, 2, 6, nodes=True)
        try:
            out = []
            for i, w in enumerate(wins):
                out.append(t.window(w, "flush"))
                out[-1]["windows_warm"] = int(t.g.stats().windows_warm)
            res[st] = out
        finally:
            t.close()
    assert [w["windows_warm"] for w in res[(0, 0)]][1] == 1, "the second window did not close warm"
    for st in SETTINGS[1:]:
        for i, (a, b) in enumerate(zip(res[st], res[(0, 0)])):
            same(f"setting {st}, warm engine, window {i}", a, b)
    check_trace_oracle(res[(1, 1)][2], "boundary_known", 2, "warm engine, the whole trace as a delta window")


def test_two_windows_in_flight():
    """windows_in_flight = 2: two windows closed back to back on their own slots and streams give the rows of the one-slot (0, 0)
    engine"""
    import torch
    wins = [_mixed(0, 40_000), _mixed(65536, 65536 + 40_000)]
    t = Twin((0, 0), topo_engine(), 1, 5)
    try:
        want = [t.window(w, "run")["rows"] for w in wins]
    finally:
        t.close()
    for st in SETTINGS[1:]:
        t = Twin(st, topo_engine(windows_in_flight=2), 1, 5)
        g = t.g
        try:
            hip = g._l                                               # (the engine's library: dlsym on its handle reaches the HIP runtime it is linked against)
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
                buf = np.zeros(len(want[i]), dtype=replay.EDGE_OUT_DTYPE)
                assert len(buf) and hip.hipMemcpy(buf.ctypes.data, ctypes.c_void_p(p), len(buf) * 64, 2) == 0
                assert _sorted(buf).tobytes() == want[i].tobytes(), (st, i)
        finally:
            t.close()
