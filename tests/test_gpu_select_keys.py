"""K7, the selection (alaz_amd/csrc/sg_sel.h), on crafted keys: the cases of tests/select_cases.py — byte ladders for every round of
k7_pick's walk, ties that run out inside a workgroup span or a 256-row tile, ±0 / ±inf / NaN / denormals against every kind of
min_value, candidate counts around k, the full sort (k = 16384 with as many candidates), random bit patterns — written over the
keyed field of a real closed window's rows on the device, then selected and compared with the sort-based references
(tests/select_by_ref.py, tests/node_trend_ref.py, tests/traffic_ref.py) over the rewritten rows: positions, row bytes and counts,
all exact.

One engine per shape has every stage a selection reads switched on; sg_window_run closes one window of n distinct edges (one request
each, tests/test_gpu_pair_tiles._on_edges) and every case of every space reuses it: a selection only reads.  The shapes are
select_cases.EDGE_SHAPES / NODE_SHAPES (tests/test_select_cases.py holds every branch of the walk reachable on each of them).

Spaces: the edge rows by score (k7_keys; score at byte 40 of 64), by lat_dev / err_dev / new (k7_keys_by; 16-byte trend rows), the
node rows by every SG_NSEL_* key (k10_keys + k_gather_sel; score at byte 132 of 136, eight-word trend rows), the node rows by every
traffic key and side (k23_keys, the host form).  The fields beside the keyed one hold other values of the same case, so a key pass
that reads a neighbouring word selects something else."""
import ctypes

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_model_scaffold import MAX_LABELS, _on_edges, _topo
from tests.helpers import CLOCK, HostShim
from tests.node_trend_ref import ref_select_nodes
from tests.select_by_ref import ref_select, ref_select_by
from tests import select_cases as sc
from tests.traffic_ref import ref_select_traffic

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
SENTINEL = 0xA5
EDGE_BYTES, NODE_BYTES = replay.EDGE_OUT_DTYPE.itemsize, engine.NODE_DTYPE.itemsize
_WINDOWS = {}


def _hip():
    import torch  # noqa: F401  (the HIP runtime the engine shares)
    hip = ctypes.CDLL(None)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    return hip


class Window:
    """one closed window on the device and what a test needs to rewrite its rows and select from them"""

    def __init__(self, shape):
        import torch
        self.torch = torch
        self.shape = shape
        topo, ops, _, _, labels = _topo()
        g = engine.ServiceGraph(max_known_nodes=shape.max_known or topo.n_nodes + 8, max_edges=shape.max_edges, layers=1, max_labels=MAX_LABELS,
                                max_outbound_ips=512, max_window_events=1 << 18, k1_variant=3)
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(1))
        HostShim().apply(g, ops); g.set_label_count(len(labels))
        g.set_trend(shift=3, warmup=1); g.set_nodes(); g.set_node_trend(shift=3, warmup=1)
        g.set_traffic_trend("nodes", shift=3, warmup=1, rate_floor=2, load_floor_ns=50_000)
        ev = _on_edges(np.arange(shape.fed), np.random.default_rng(900 + shape.fed))
        while g.ingest(ev) != 0:
            pass
        g.window_run()
        self.g = g
        self.rows = g.window_read().copy()                            # (the window is now the last read one too: the host forms' slot)
        torch.cuda.synchronize()
        self.hip = _hip()                                             # (after the engine and torch have the HIP runtime loaded)
        self.E = len(self.rows)
        self.p_rows, self.p_trend = g.rows_buffer(), g.trend_buffer()
        self.p_nodes, p_count = g.nodes_buffer()
        self.p_ntrend, self.p_traffic = g.node_trend_buffer(), g.window_traffic_buffer("nodes")
        self.N = int(self.read(p_count, 1, np.uint64)[0])
        assert self.read(self.p_rows, self.E, replay.EDGE_OUT_DTYPE).tobytes() == self.rows.tobytes()
        self.trend = self.read(self.p_trend, self.E, engine.TREND_DTYPE)
        self.nodes = self.read(self.p_nodes, self.N, engine.NODE_DTYPE)
        self.ntrend = self.read(self.p_ntrend, self.N, engine.NODE_TREND_DTYPE)
        self.traffic = self.read(self.p_traffic, self.N, engine.NODE_TREND_DTYPE)
        assert self.nodes.tobytes() == g.window_nodes().tobytes() and self.ntrend.tobytes() == g.window_node_trend().tobytes()
        assert self.E == shape.E and self.N == (self.N if shape.N is None else shape.N), (shape, self.E, self.N)
        assert -(-shape.max_edges // 2048) == shape.spans and -(-g.window_buffers()[3] // 2048) == shape.node_spans
        cap = max(self.E, self.N, 1)
        self.d_out = torch.zeros(cap * NODE_BYTES, dtype=torch.uint8, device="cuda")
        self.d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
        self.d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def read(self, ptr, n, dtype):
        out = np.zeros(n, dtype=dtype)
        if n:
            assert self.hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, D2H) == 0
        return out

    def write(self, ptr, a):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            assert self.hip.hipMemcpy(ctypes.c_void_p(ptr), a.ctypes.data, a.nbytes, H2D) == 0

    def select(self, call, row_bytes, cap, sentinel=False):
        """call(d_out, d_idx, cap, d_n) enqueues a device-form selection: (count, indices written, row bytes written); with
        sentinel the whole buffers come back, pre-filled, so that what lies beyond cap shows"""
        t = self.torch
        if sentinel:
            self.write(self.d_out.data_ptr(), np.full(self.d_out.numel(), SENTINEL, np.uint8))
            self.write(self.d_idx.data_ptr(), np.full(self.d_idx.numel(), -1, np.int32))
        call(self.d_out.data_ptr(), self.d_idx.data_ptr(), cap, self.d_n.data_ptr())
        t.cuda.synchronize()
        n = int(self.read(self.d_n.data_ptr(), 1, np.int64)[0])
        m = self.d_idx.numel() if sentinel else min(n, cap)
        return n, self.read(self.d_idx.data_ptr(), m, np.int32).astype(np.uint32), self.read(self.d_out.data_ptr(), m * row_bytes, np.uint8)


def _window(shape) -> Window:
    if shape not in _WINDOWS:
        _WINDOWS[shape] = Window(shape)
    return _WINDOWS[shape]


def _ids(shapes):
    return [f"E{s.E}-N{s.N}" for s in shapes]


def _families(shape, full):
    """the whole case list on the shapes in `full`, ties and specials on every shape"""
    return sc.FAMILIES if shape in full else ("ties", "specials")


def _other(values, j):
    """other values of the same case for the fields beside the keyed one: the case's values rotated by j rows and negated"""
    return -np.roll(values, j)


def _compare(got, want, rows, row_bytes, what):
    n, idx, out = got
    assert n == len(want), (what, n, len(want))
    assert np.array_equal(idx, want), what
    assert out.tobytes() == rows[want].tobytes(), what


def _check_caps(w, call, row_bytes, rows, want, what):
    """a cap below the number selected: the count is the full selection's, the first cap rows and indices are written, nothing else"""
    assert len(want) > 1, what
    for cap in (1, len(want) - 1):
        n, idx, out = w.select(call, row_bytes, cap, sentinel=True)
        assert n == len(want), (what, cap)
        assert np.array_equal(idx[:cap], want[:cap]) and (idx[cap:] == 0xFFFFFFFF).all(), (what, cap)
        assert out[: cap * row_bytes].tobytes() == rows[want[:cap]].tobytes() and (out[cap * row_bytes:] == SENTINEL).all(), (what, cap)


FULL_EDGES = sc.EDGE_SHAPES                                                        # the score space runs every case on every shape
FULL_BY = tuple(s for s in sc.EDGE_SHAPES if s.E in (2049, 20_000))
FULL_NODES = tuple(s for s in sc.NODE_SHAPES if s.E in (2049, 20_000))


# ---- the edge rows by score: k7_keys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.EDGE_SHAPES, ids=_ids(sc.EDGE_SHAPES))
def test_edges_by_score(shape):
    w = _window(shape)
    g, E = w.g, w.E
    seen = 0
    for c in sc.cases(E, shape.spans, _families(shape, FULL_EDGES)):
        rows = w.rows.copy()
        rows["score"], rows["lat_z"], rows["err_ratio"] = c.values, _other(c.values, 1), _other(c.values, 2)
        rows["err_count"] = _other(c.values, 3).view(np.uint32)                   # (the word before the score)
        w.write(w.p_rows, rows)
        want = ref_select(rows, c.k, c.min_value)
        _compare(w.select(lambda o, i, cap, n: g.window_select(c.k, c.min_value, o, i, cap, n, 0), EDGE_BYTES, max(E, 1)), want, rows, EDGE_BYTES, c.name)
        seen += 1
    assert seen > 40
    # a cap below the selection, threshold mode and top-k mode
    rows = w.rows.copy()
    rows["score"] = np.random.default_rng(E).permutation(E).astype(np.float32)
    w.write(w.p_rows, rows)
    for k, mv in ((0, sc.NEG_INF), (min(E, 1000), sc.NEG_INF), (0, float(E // 2))):
        want = ref_select(rows, k, mv)
        if len(want) > 1:
            _check_caps(w, lambda o, i, cap, n: g.window_select(k, mv, o, i, cap, n, 0), EDGE_BYTES, rows, want, (k, mv))
    w.write(w.p_rows, w.rows)


# ---- the edge rows by a trend key: k7_keys_by -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["lat_dev", "err_dev"])
@pytest.mark.parametrize("shape", sc.EDGE_SHAPES, ids=_ids(sc.EDGE_SHAPES))
def test_edges_by_a_trend_value(shape, by):
    w = _window(shape)
    g, E = w.g, w.E
    other = "err_dev" if by == "lat_dev" else "lat_dev"
    w.write(w.p_rows, w.rows)
    for c in sc.cases(E, shape.spans, _families(shape, FULL_BY)):
        tr = w.trend.copy()
        tr[by], tr[other], tr["base_mean_us"] = c.values, _other(c.values, 1), _other(c.values, 2)
        tr["windows_seen"] = _other(c.values, 3).view(np.uint32)
        w.write(w.p_trend, tr)
        want = ref_select_by(w.rows, tr, by, c.k, c.min_value)
        _compare(w.select(lambda o, i, cap, n: g.window_select(c.k, c.min_value, o, i, cap, n, 0, by=by), EDGE_BYTES, max(E, 1)), want, w.rows,
                 EDGE_BYTES, (by, c.name))
    tr = w.trend.copy()
    tr[by] = np.random.default_rng(E).permutation(E).astype(np.float32)
    w.write(w.p_trend, tr)
    for k in (0, min(E, 300)):
        want = ref_select_by(w.rows, tr, by, k, 1.0)
        if len(want) > 1:
            _check_caps(w, lambda o, i, cap, n: g.window_select(k, 1.0, o, i, cap, n, 0, by=by), EDGE_BYTES, w.rows, want, (by, k))


@pytest.mark.parametrize("shape", sc.EDGE_SHAPES, ids=_ids(sc.EDGE_SHAPES))
def test_edges_by_new(shape):
    """one key for every row with windows_seen == 0 and a request: all ties, by position.  The rows that are not new are so for
    either reason — seen before (any bit of the word), or no request (an alive-only row)"""
    w = _window(shape)
    g, E = w.g, w.E
    ar = np.arange(E)
    for name, mask, k in sc.new_masks(E, shape.spans):
        rows, tr = w.rows.copy(), w.trend.copy()
        kind = ar % 3                                                              # not new: no request; seen (the top bit); both
        rows["count"] = np.where(mask, 1 + kind, np.where(kind == 1, 7, 0))
        tr["windows_seen"] = np.where(mask, 0, np.where(kind == 0, 0, np.where(kind == 1, 1 << 31, 1)))
        tr["lat_dev"], tr["err_dev"] = ar[::-1], -ar                               # (values that would order the rows otherwise)
        w.write(w.p_rows, rows); w.write(w.p_trend, tr)
        want = ref_select_by(rows, tr, "new", k, 0.0)
        assert len(want) == (min(k, int(mask.sum())) if k else int(mask.sum())), name
        _compare(w.select(lambda o, i, cap, n: g.window_select(k, 0.0, o, i, cap, n, 0, by="new"), EDGE_BYTES, max(E, 1)), want, rows, EDGE_BYTES, name)
    rows["count"], tr["windows_seen"] = 1 + ar % 5, np.where(ar % 3 == 1, 4, 0)    # two rows of three are new
    w.write(w.p_rows, rows); w.write(w.p_trend, tr)
    for k in (0, min(E // 2, 300)):                                                # a cap below the selection, both modes
        want = ref_select_by(rows, tr, "new", k, 0.0)
        if len(want) > 1:
            _check_caps(w, lambda o, i, cap, n: g.window_select(k, 0.0, o, i, cap, n, 0, by="new"), EDGE_BYTES, rows, want, ("new caps", k))
    w.write(w.p_rows, w.rows)


# ---- the node rows by every SG_NSEL_* key: k10_keys and k_gather_sel --------------------------------------------------------------------------
NODE_DEVS = ("in_lat_dev", "in_err_dev", "out_lat_dev", "out_err_dev")


@pytest.mark.parametrize("by", ["score"] + list(NODE_DEVS))
@pytest.mark.parametrize("shape", sc.NODE_SHAPES, ids=_ids(sc.NODE_SHAPES))
def test_nodes_by_every_value_key(shape, by):
    assert set(engine.NSEL_BY) == {"score", "new", *NODE_DEVS}
    w = _window(shape)
    g, N = w.g, w.N
    capped = set()
    for c in sc.cases(N, shape.node_spans, _families(shape, FULL_NODES)):
        nodes, tr = w.nodes.copy(), w.ntrend.copy()
        if by == "score":
            nodes["score"], nodes["in_score_max"], nodes["out_score_max"] = c.values, _other(c.values, 1), _other(c.values, 2)
        else:
            for j, f in enumerate(NODE_DEVS + ("in_base_mean_us", "out_base_mean_us")):
                tr[f] = c.values if f == by else _other(c.values, j + 1)
            nodes["score"] = _other(c.values, 7)
        w.write(w.p_nodes, nodes); w.write(w.p_ntrend, tr)
        want = ref_select_nodes(nodes, tr, by, c.k, c.min_value)
        call = lambda o, i, cap, n, c=c: g.window_nodes_select(c.k, c.min_value, o, i, cap, n, 0, by=by)   # noqa: E731
        _compare(w.select(call, NODE_BYTES, max(N, 1)), want, nodes, NODE_BYTES, (by, c.name))
        if len(want) > 2 and (c.k == 0) not in capped:                             # one threshold-mode case and one top-k case
            capped.add(c.k == 0)
            _check_caps(w, call, NODE_BYTES, nodes, want, (by, c.name, "caps"))
    assert N < 20 or capped == {True, False}
    # the host form on the last case: the same positions and rows
    sel, idx, nn = g.window_nodes_top(c.k, c.min_value, by=by, cap=max(N, 1))
    assert nn == N and np.array_equal(idx, want) and sel.tobytes() == nodes[want].tobytes()
    w.write(w.p_nodes, w.nodes); w.write(w.p_ntrend, w.ntrend)


@pytest.mark.parametrize("shape", sc.NODE_SHAPES, ids=_ids(sc.NODE_SHAPES))
def test_nodes_by_new(shape):
    """new: in_seen == 0, out_seen == 0 and a request on either side (the two 64-bit counts, either half of either).  The rows that
    are not new are so for each reason in turn"""
    w = _window(shape)
    g, N = w.g, w.N
    ar = np.arange(N, dtype=np.uint64)
    capped = set()
    for name, mask, k in sc.new_masks(N, shape.node_spans):
        nodes, tr = w.nodes.copy(), w.ntrend.copy()
        kind = ar % 3
        nodes["in_count"] = np.where(mask, np.where(kind == 0, 5, np.where(kind == 1, 0, np.uint64(1) << np.uint64(32))), np.where(kind == 0, 0, 9))
        nodes["out_count"] = np.where(mask, np.where(kind == 1, 3, 0), np.where(kind == 0, 0, 2))
        tr["in_seen"] = np.where(mask, 0, np.where(kind == 1, 1 << 31, 0))
        tr["out_seen"] = np.where(mask, 0, np.where(kind == 2, 1, 0))
        nodes["score"] = ar[::-1].astype(np.float32)
        w.write(w.p_nodes, nodes); w.write(w.p_ntrend, tr)
        want = ref_select_nodes(nodes, tr, "new", k, 0.0)
        assert len(want) == (min(k, int(mask.sum())) if k else int(mask.sum())), name
        call = lambda o, i, cap, n, k=k: g.window_nodes_select(k, 0.0, o, i, cap, n, 0, by="new")   # noqa: E731
        _compare(w.select(call, NODE_BYTES, max(N, 1)), want, nodes, NODE_BYTES, name)
        if len(want) > 2 and "half" in name and k in (0, int(mask.sum()) - 1):      # a cap below the selection, both modes
            _check_caps(w, call, NODE_BYTES, nodes, want, (name, "caps"))
            capped.add(k == 0)
    assert N < 20 or capped == {True, False}
    w.write(w.p_nodes, w.nodes); w.write(w.p_ntrend, w.ntrend)


# ---- the node rows by a traffic key: k23_keys ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("by", list(engine.TSEL_BY))
@pytest.mark.parametrize("shape", sc.NODE_SHAPES, ids=_ids(sc.NODE_SHAPES))
def test_nodes_by_traffic(shape, by, side):
    """surge / load_up rank the side's lat_dev / err_dev word, drop / load_down the same word with its sign bit flipped: the word
    holds the case's values with the sign bit flipped back, so K7 sees the case's keys either way — a flipped NaN stays out, the
    two zeros stay one key"""
    assert set(engine.TSEL_BY) == {"surge", "drop", "load_up", "load_down"}
    w = _window(shape)
    g, N = w.g, w.N
    falling = by in ("drop", "load_down")
    word = f"{side}_{'lat_dev' if by in ('surge', 'drop') else 'err_dev'}"
    w.write(w.p_nodes, w.nodes)
    full = shape in FULL_NODES and (by, side) in (("drop", "in"), ("load_up", "out"))
    for c in sc.cases(N, shape.node_spans, sc.FAMILIES if full else ("ties", "specials")):
        tr = w.traffic.copy()
        for j, f in enumerate(NODE_DEVS + ("in_base_mean_us", "out_base_mean_us")):
            tr[f] = _other(c.values, j + 1)
        tr[word] = (c.values.view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32) if falling else c.values
        w.write(w.p_traffic, tr)
        want = ref_select_traffic(tr, by, side, c.k, c.min_value)
        vals = np.zeros(N, dtype=[("v", "<f4")]); vals["v"] = c.values
        assert np.array_equal(want, ref_select_by(None, vals, "v", c.k, c.min_value)), c.name   # (the signed column is the case)
        sel, idx, nn = g.window_nodes_top_traffic(c.k, c.min_value, by=by, side=side, cap=max(N, 1))
        assert nn == N and np.array_equal(idx, want), (by, side, c.name)
        assert sel.tobytes() == w.nodes[want].tobytes(), (by, side, c.name)
    assert g.window_node_traffic().tobytes() == tr.tobytes()           # the slot written is the one the host forms read
    if len(want) > 1:                                                  # the host form's cap: the first rows, the full count is not reported
        sel, idx, nn = g.window_nodes_top_traffic(c.k, c.min_value, by=by, side=side, cap=len(want) - 1)
        assert np.array_equal(idx, want[:-1]) and sel.tobytes() == w.nodes[want[:-1]].tobytes()
    w.write(w.p_traffic, w.traffic)
