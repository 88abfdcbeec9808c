"""The front end's methods of the latency percentiles (K20) against the recording stand-in of tests/test_engine_front.py: the C calls
they make (argument order, buffers inside numpy arrays), the shapes and dtypes they return, the default {500, 990}, and the texts of
their errors."""

import numpy as np
import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern = front.same, front.pattern
H, I, O, U4 = front.H, front.I, front.O, front.U4
HIST2, HIST1 = np.dtype(("<u8", (2, 16))), np.dtype(("<u8", (16,)))
NEW_ABI = {
    "sg_set_quantiles": [H, I, front.In(U4, 3), I],
    "sg_window_node_hist": front._INDEXED(HIST2), "sg_window_group_hist": front._INDEXED(HIST1),
    "sg_window_group_node_hist": front._INDEXED(HIST2),
    # (the quantile rows' size follows n_q: the stand-in checks the buffer for the largest, and each test for its own)
    "sg_window_node_quantiles": front._INDEXED(np.dtype(("<u4", (2, 1)))), "sg_window_group_quantiles": front._INDEXED(np.dtype(("<u4", (1,)))),
    "sg_window_group_node_quantiles": front._INDEXED(np.dtype(("<u4", (2, 1)))),
    "sg_window_quantiles_buffer": [H, I, O, O],
}


g = front.abi_fixture(NEW_ABI)


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 8
    for name in NEW_ABI:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    for name in NEW_ABI:
        if name.startswith("sg_window_") and name.endswith(("_hist", "_quantiles")):
            assert engine._SIGNATURES[name] == engine._SIGNATURES["sg_window_node_trend"], name   # the indexed readbacks' shape
    assert engine.ABI_VERSION == 6 and engine.Q_SPACES == dict(nodes=1, groups=2, group_nodes=4) and engine.Q_MAX == 8
    assert not [n for n in dir(engine) if n.endswith("_DTYPE") and "QUANT" in n]   # plain arrays: no struct twin, no dtype constant


def test_set_quantiles(g):
    cfn = "sg_set_quantiles"
    g.set_quantiles()                                                  # the node space, {500, 990}
    g.set_quantiles(("nodes", "groups", "group_nodes"), (1, 1000, 999))
    g.set_quantiles("groups", [750])
    g.set_quantiles(6, ())                                             # bits as an int; no per-mille: the library's default
    g.set_quantiles(None)
    assert g._l.take() == [(cfn, "h", 1, ("in", [500, 990]), 2), (cfn, "h", 7, ("in", [1, 1000, 999]), 3), (cfn, "h", 2, ("in", [750]), 1),
                           (cfn, "h", 6, None, 0), (cfn, "h", 0, ("in", [500, 990]), 2)]
    with pytest.raises(ValueError) as ei:
        g.set_quantiles(("nodes", "pods"))
    assert "unknown quantile space 'pods'" in str(ei.value) and g._l.take() == []
    text = b"sg_set_quantiles: the engine was created without SG_CFG_EDGE_HISTOGRAM"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_quantiles("nodes", (500,))
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


HISTS = [("window_node_hist", "sg_window_node_hist", HIST2), ("window_group_hist", "sg_window_group_hist", HIST1),
         ("window_group_node_hist", "sg_window_group_node_hist", HIST2)]
QUANTS = [("window_node_quantiles", "sg_window_node_quantiles", 2), ("window_group_quantiles", "sg_window_group_quantiles", 1),
          ("window_group_node_quantiles", "sg_window_group_node_quantiles", 2)]


def _indexed(g, method, cfn, dtype):
    call = getattr(g, method)
    same(call(), dtype, pattern(dtype, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(call(index=None), dtype, pattern(dtype, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    g._l.script[cfn] = dict(out=[2])
    same(call(index=[2, 0]), dtype, pattern(dtype, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    same(call(index=[]), dtype, pattern(dtype, 0))
    assert g._l.take() == []
    text = cfn.encode() + b": a node index beyond the window's nodes"
    g._l.script = {cfn: dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(index=[9])
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith(text.decode())


@pytest.mark.parametrize("method,cfn,dtype", HISTS, ids=[c[0] for c in HISTS])
def test_histogram_readbacks(g, method, cfn, dtype):
    _indexed(g, method, cfn, dtype)
    g._l.script = {cfn: dict(out=[5])}
    a = getattr(g, method)()
    assert a.dtype == np.uint64 and a.shape == (5,) + dtype.shape


@pytest.mark.parametrize("n_q", [None, 1, 3, 8])
@pytest.mark.parametrize("method,cfn,sides", QUANTS, ids=[c[0] for c in QUANTS])
def test_quantile_readbacks_follow_n_q(g, monkeypatch, method, cfn, sides, n_q):
    """the rows are [2][n_q] (or [n_q]) u32: n_q as the last set_quantiles recorded it, 2 before any"""
    if n_q is not None:
        g.set_quantiles("nodes", tuple(range(1, n_q + 1))); g._l.take()
    nq = n_q or 2
    dtype = np.dtype(("<u4", (2, nq) if sides == 2 else (nq,)))
    monkeypatch.setitem(front.ABI, cfn, front._INDEXED(dtype))         # the stand-in checks the buffers for this row size
    _indexed(g, method, cfn, dtype)
    g._l.script = {cfn: dict(out=[4])}
    a = getattr(g, method)()
    assert a.dtype == np.uint32 and a.shape == (4,) + dtype.shape


def test_window_quantiles_buffer(g):
    cfn = "sg_window_quantiles_buffer"
    g._l.script = {cfn: dict(out=[0x1000, 0x2000])}
    assert g.window_quantiles_buffer("groups") == (0x1000, 0x2000) == g.window_quantiles_buffer(4)
    assert g._l.take() == [(cfn, "h", 2, "out", "out"), (cfn, "h", 4, "out", "out")]
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_quantiles_buffer("nodes")
    assert str(ei.value) == "servicegraph rc=-71: off"
