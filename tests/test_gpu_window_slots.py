"""Which window slot each reader addresses (alaz_amd/csrc/servicegraph.hip, DESIGN.md "Windows in flight"): an engine with 1, 2 or 3
window slots runs four windows through sg_window_run; after every window each reader is compared with a one-slot engine that ran
the same windows.

Two slots are in play after window i (0-based) of an engine with NW slots:
  ran last — the slot window i ran in, i % NW: sg_window_rows_buffer, sg_window_select and every *_buffer call read it.
  working  — the slot the next batch goes to, (i + 1) % NW: sg_window_read and the host readers (sg_window_trend, sg_window_nodes,
             sg_window_node_trend, sg_window_rank, sg_window_nodes_top, sg_window_rank_top) read it.  With one slot the two are
             the same.  With more, the working slot holds what window i + 1 - NW left there, or nothing yet.

This records what the engine does, oddities included: with two or more slots sg_window_read after sg_window_run is refused
(SG_ESTATE: the working slot is not the one that ran last), sg_window_trend returns no rows (its count is the last READ window's
edge count, and nothing was read), and the other host readers return the rows of window i + 1 - NW, or SG_ESTATE before the
working slot has run a window.

The graph is the smallest at which a slot mix-up shows: 36 nodes, 1 500 events a window, one layer, four windows of different
events."""

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _d2h, _hip, _rc
from tests.helpers import CLOCK, HostShim

pytestmark = pytest.mark.gpu

LAYERS = 1
WINDOWS = 4
TOP_K = 5
SEL_K = 50
CAP = 2048                                                            # = max_edges: no selection is cut
KINDS = {"warm3": dict(k1_variant=3, warm=True), "table1": dict(k1_variant=1)}
NEG_INF = float("-inf")

_TRACE = {}


def _trace():
    if not _TRACE:
        topo = replay.make_topology(24, 200, seed=701, svcs=12)
        wins, labels = [], None
        for i in range(WINDOWS):
            ev, labels = replay.make_events(topo, 1_500, seed=702 + i, fixed_labels=True)
            wins.append(np.ascontiguousarray(ev))
        assert len({w.tobytes() for w in wins}) == WINDOWS
        _TRACE.update(topo=topo, labels=labels, wins=wins)
    return _TRACE["topo"], _TRACE["labels"], _TRACE["wins"]


def _engine(kind, in_flight):
    topo, labels, _ = _trace()
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 16, max_edges=CAP, layers=LAYERS, max_labels=256, max_outbound_ips=512,
                            max_window_events=1 << 16, windows_in_flight=in_flight, **KINDS[kind])
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(LAYERS))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_trend(shift=3, warmup=1, ttl=4)
    g.set_nodes(); g.set_node_trend(shift=3, warmup=1, ttl=4); g.set_rank(iters=5)
    return g


class Run:
    """one engine and the device memory it selects into; window(i) runs window i and returns what the readers of the slot that ran
    last give"""
    def __init__(self, kind, in_flight):
        import torch
        self.g = _engine(kind, in_flight)                              # (first: loading the engine makes the HIP runtime's symbols global)
        self.torch, self.hip = torch, _hip()
        self.dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in _trace()[2]]
        self.d_out = torch.zeros(CAP * 64, dtype=torch.uint8, device="cuda")
        self.d_idx = torch.zeros(CAP, dtype=torch.int32, device="cuda")
        self.d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def window(self, i, n_edges=None):
        """n_edges None (the one-slot reference): the window is read (sg_window_read) for its edge count, the rows come back as `read`"""
        g, hip = self.g, self.hip
        g.ingest_device(self.dev[i].data_ptr(), len(_trace()[2][i]), 0)
        g.window_run(0)
        ptr = g.rows_buffer()
        g.window_select(SEL_K, NEG_INF, self.d_out.data_ptr(), self.d_idx.data_ptr(), CAP, self.d_n.data_ptr(), 0)
        tp, ntp, rp, (np_, cp) = g.trend_buffer(), g.node_trend_buffer(), g.rank_buffer(), g.nodes_buffer()
        self.torch.cuda.synchronize()
        read = None
        if n_edges is None:
            read = g.window_read().copy()
            n_edges = len(read)
        m = int(self.d_n.item())
        cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
        return dict(ptr=ptr, read=read, rows=_d2h(hip, ptr, n_edges, replay.EDGE_OUT_DTYPE), sel_n=m,
                    sel_idx=self.d_idx.cpu().numpy()[:m].astype(np.uint32), sel_rows=self.d_out.cpu().numpy()[: m * 64].tobytes(),
                    trend=_d2h(hip, tp, n_edges, engine.TREND_DTYPE), nodes=_d2h(hip, np_, cnt, engine.NODE_DTYPE),
                    node_trend=_d2h(hip, ntp, cnt, engine.NODE_TREND_DTYPE), rank=_d2h(hip, rp, cnt, engine.RANK_DTYPE))

    def host(self):
        """what the host readers give now"""
        g = self.g
        top, top_idx, top_nn = g.window_nodes_top(TOP_K)
        rt, rt_rank, rt_idx, rt_nn = g.window_rank_top(TOP_K)
        return dict(nodes=g.window_nodes(), node_trend=g.window_node_trend(), rank=g.window_rank(),
                    top=(top.tobytes(), top_idx.tolist(), top_nn), rank_top=(rt.tobytes(), rt_rank.tobytes(), rt_idx.tolist(), rt_nn))


_REF = {}


def _reference(kind):
    """the one-slot engine's windows, made once per kind: per window what the device readers give (`dev`), the rows sg_window_read
    returns and what the host readers give — with one slot all of them address the same window"""
    if kind not in _REF:
        r = Run(kind, 1)
        try:
            out = []
            for i in range(WINDOWS):
                d = r.window(i)
                w = dict(dev=d, read=d["read"], host_trend=r.g.window_trend(), **r.host())
                assert d["rows"].tobytes() == w["read"].tobytes() and len(w["read"]) > 100
                assert d["nodes"].tobytes() == w["nodes"].tobytes() and d["rank"].tobytes() == w["rank"].tobytes()
                assert d["trend"].tobytes() == w["host_trend"].tobytes() and d["node_trend"].tobytes() == w["node_trend"].tobytes()
                assert d["sel_n"] == SEL_K and len(d["nodes"]) > 20
                out.append(w)
            assert len({w["read"].tobytes() for w in out}) == WINDOWS and len({w["rank"].tobytes() for w in out}) == WINDOWS
            _REF[kind] = out
        finally:
            r.g.close()
    return _REF[kind]


@pytest.mark.parametrize("in_flight", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_each_reader_addresses_its_slot(kind, in_flight):
    ref = _reference(kind)
    r = Run(kind, in_flight)
    g = r.g
    try:
        ptrs = []
        for i in range(WINDOWS):
            want = ref[i]
            d = r.window(i, len(want["read"]))
            ptrs.append(d["ptr"])
            # the slot that ran last: window i, whatever the number of slots
            assert d["rows"].tobytes() == want["read"].tobytes(), i
            assert d["sel_n"] == want["dev"]["sel_n"] and d["sel_idx"].tolist() == want["dev"]["sel_idx"].tolist(), i
            assert d["sel_rows"] == want["dev"]["sel_rows"] == want["read"][d["sel_idx"]].tobytes(), i
            for what in ("nodes", "trend", "node_trend", "rank"):
                assert d[what].tobytes() == want["dev"][what].tobytes(), (i, what)
            # the working slot
            if in_flight == 1:
                assert g.window_read().tobytes() == want["read"].tobytes(), i
                assert g.window_trend().tobytes() == want["host_trend"].tobytes(), i
            else:
                assert _rc(g.window_read) == engine.SG_ESTATE, i
                assert len(g.window_trend()) == 0, i
            j = i + 1 - in_flight                                      # the window the working slot ran last
            if j < 0:
                for call in (g.window_nodes, g.window_node_trend, g.window_rank):
                    assert _rc(call) == engine.SG_ESTATE, (i, call)
                assert _rc(g.window_nodes_top, TOP_K) == engine.SG_ESTATE and _rc(g.window_rank_top, TOP_K) == engine.SG_ESTATE
            else:
                got = r.host()
                for what in ("nodes", "node_trend", "rank"):
                    assert got[what].tobytes() == ref[j][what].tobytes(), (i, j, what)
                assert got["top"] == ref[j]["top"] and got["rank_top"] == ref[j]["rank_top"], (i, j)
        assert len(set(ptrs)) == in_flight and all(ptrs[i] == ptrs[i % in_flight] for i in range(WINDOWS))
    finally:
        g.close()
