"""Node selection (sg_window_nodes_top / sg_window_nodes_select): K7 over the node rows by every key of NSEL_BY, against the numpy
reference tests/node_trend_ref.ref_select_nodes over the same window's node rows and node trend rows; the host form and the device
form select the same nodes, and the rows are byte-identical to sg_window_nodes's."""
import ctypes

import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import PARAMS, _engine, _feed, _hip, _rc
from tests.node_trend_ref import ref_select_nodes
from tests.traces import churn  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

BY = list(engine.NSEL_BY)


def _ks(n_cand):
    return sorted({0, 1, 100, n_cand + 5, engine.SELECT_MAX_K})


def _thresholds(v):
    v = v[np.isfinite(v)]
    if not len(v):
        return [float("-inf")]
    return [float("-inf"), 0.0, float(np.median(v)), float(v.max())]


def _check_top(g, nodes, tr, by, k, t):
    sel, idx, nn = g.window_nodes_top(k, t, by=by)
    want = ref_select_nodes(nodes, tr, by, k, t)
    assert nn == len(nodes)
    assert idx.tolist() == want.tolist(), (by, k, t)
    assert sel.tobytes() == nodes[want].tobytes()
    if by != "score" and len(idx):
        assert g.window_node_trend(idx).tobytes() == tr[idx].tobytes()
    return want


def test_every_key_k_and_threshold_against_the_reference(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    checked = {b: 0 for b in BY}
    for i, w in enumerate(wins[:7]):
        _feed(g, w)
        g.flush_window()
        nodes, tr = g.window_nodes(), g.window_node_trend()
        for by in BY:
            v = nodes["score"] if by == "score" else tr[by] if by != "new" else None
            ths = [0.0] if by == "new" else _thresholds(v)
            for t in ths:
                n_cand = len(ref_select_nodes(nodes, tr, by, 0, t))
                for k in _ks(n_cand):
                    if _check_top(g, nodes, tr, by, k, t).size:
                        checked[by] += 1
    assert all(checked.values()), checked


def test_ties_and_small_caps(churn):
    """many equal values (the new nodes all share one key): ties go by node position; a cap below the count returns the first cap
    of the order"""
    topo, labels, wins = churn
    g = _engine(topo, labels)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    _feed(g, wins[0]); g.flush_window()
    nodes, tr = g.window_nodes(), g.window_node_trend()
    want = ref_select_nodes(nodes, tr, "new", 0, 0.0)
    assert len(want) == len(nodes) - int(((nodes["in_count"] | nodes["out_count"]) == 0).sum()) > 100   # every node is new
    for k in (1, 7, 100):
        _check_top(g, nodes, tr, "new", k, 0.0)
    for k in (0, 50):
        sel, idx, nn = g.window_nodes_top(k, 0.0, cap=10)
        full = ref_select_nodes(nodes, None, "score", k, 0.0)
        assert idx.tolist() == full[:10].tolist() and sel.tobytes() == nodes[full[:10]].tobytes()


def test_device_form_matches_the_host_form(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, windows_in_flight=2)
    g.set_nodes(); g.set_node_trend(**PARAMS)
    hip = _hip()
    cap = 4096
    d_out = torch.zeros(cap * engine.NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:6]):
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        np_, cp = g.nodes_buffer()
        tp = g.node_trend_buffer()
        torch.cuda.synchronize()
        cnt = np.zeros(1, np.uint64)
        assert hip.hipMemcpy(cnt.ctypes.data, ctypes.c_void_p(cp), 8, 2) == 0
        nodes = np.zeros(int(cnt[0]), engine.NODE_DTYPE)
        assert hip.hipMemcpy(nodes.ctypes.data, ctypes.c_void_p(np_), nodes.nbytes, 2) == 0
        tr = np.zeros(len(nodes), engine.NODE_TREND_DTYPE)
        assert hip.hipMemcpy(tr.ctypes.data, ctypes.c_void_p(tp), tr.nbytes, 2) == 0
        for by in BY:
            for k, t in ((0, 0.0), (1, float("-inf")), (100, 0.0), (engine.SELECT_MAX_K, float("-inf"))):
                g.window_nodes_select(k, t, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0, by=by)
                torch.cuda.synchronize()
                m = int(d_n.cpu()[0])
                want = ref_select_nodes(nodes, tr, by, k, t)
                assert m == len(want), (by, k, t)
                take = min(m, cap)
                assert d_idx.cpu().numpy()[:take].astype(np.uint32).tolist() == want[:take].tolist()
                got = d_out.cpu().numpy()[: take * engine.NODE_DTYPE.itemsize].tobytes()
                assert got == nodes[want[:take]].tobytes()
        # rows only (no index array)
        g.window_nodes_select(5, float("-inf"), d_out.data_ptr(), 0, cap, d_n.data_ptr(), 0)
        torch.cuda.synchronize()
        want = ref_select_nodes(nodes, None, "score", 5, float("-inf"))
        assert d_out.cpu().numpy()[: len(want) * engine.NODE_DTYPE.itemsize].tobytes() == nodes[want].tobytes()


def test_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.window_nodes_top, 1) == engine.SG_ESTATE              # the rollup is off
    g.set_nodes()
    _feed(g, wins[0]); g.flush_window()
    assert len(g.window_nodes_top(1)[0]) == 1                          # the score needs only the rollup
    for by in BY[1:]:
        assert _rc(g.window_nodes_top, 1, by=by) == engine.SG_ESTATE    # a trend key with the node trend off
    assert g._l.sg_window_nodes_top(g._h, 6, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    assert g._l.sg_window_nodes_top(g._h, 0, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    g.set_node_trend(**PARAMS)
    assert _rc(g.window_nodes_top, 1, by="in_lat_dev") == engine.SG_ESTATE   # the read window was closed before it was on
    _feed(g, wins[1])
    g.flush_begin()
    assert _rc(g.window_nodes_top, 1) == engine.SG_ESTATE              # a flush is open
    g.flush_end()
    for by in BY:
        g.window_nodes_top(3, by=by)
