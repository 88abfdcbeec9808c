"""The front end's methods of the tail baselines (K21) against the recording stand-in of tests/test_engine_front.py: the C calls they
make (argument order, buffers inside numpy arrays), the dtypes they return, the texts of their errors, and that the stage adds
functions only — no struct, no dtype, no constant set."""
import ctypes as C
import struct

import pytest

from alaz_amd import engine
from tests.abi_layouts import LAYOUTS
from tests import engine_front as front

same, pattern, INF = front.same, front.pattern, front.INF
H, I, F, O, S, SO, U4, Out = front.H, front.I, front.F, front.O, front.S, front.SO, front.U4, front.Out
TOP = lambda dt: [H, I, I, F, Out(dt, 6), Out(U4, 6), I, O, O]     # f(h, by, k, min_value, out, index, cap, *n_selected, *n_rows)
NEW_ABI = {
    "sg_set_quantile_trend": [H, I, I, S],
    "sg_window_node_quantile_trend": front._INDEXED(engine.NODE_TREND_DTYPE),
    "sg_window_group_quantile_trend": front._INDEXED(engine.TREND_DTYPE),
    "sg_window_group_node_quantile_trend": front._INDEXED(engine.NODE_TREND_DTYPE),
    "sg_window_quantile_trend_buffer": [H, I, O],
    "sg_quantile_trend_entries": [H, I, Out(engine.TREND_ENTRY_DTYPE, 3), I, O],
    "sg_quantile_trend_stats_get": [H, I, SO],
    "sg_window_nodes_top_tail": TOP(engine.NODE_DTYPE), "sg_window_groups_top_tail": TOP(engine.GROUP_EDGE_DTYPE),
    "sg_window_group_nodes_top_tail": TOP(engine.NODE_DTYPE),
    "sg_window_group_nodes": front._COUNTED(engine.NODE_DTYPE),
}
METHODS = ("set_quantile_trend", "window_node_quantile_trend", "window_group_quantile_trend", "window_group_node_quantile_trend",
           "window_quantile_trend_buffer", "quantile_trend_entries", "quantile_trend_stats", "window_nodes_top_tail", "window_groups_top_tail",
           "window_group_nodes_top_tail")
_TREND = [("shift", 4), ("warmup", 4), ("ttl", 64), ("max_entries", 0), ("lat_floor_ns", 1000), ("err_floor", 10486)]


def _packed(**over):
    return struct.pack("<4I2Q2I", 40, *[over.get(f, d) for f, d in _TREND], 0)


g = front.abi_fixture(NEW_ABI)


def test_ten_functions_and_nothing_else():
    new = [n for n in NEW_ABI if n != "sg_window_group_nodes"]
    assert len(new) == 10 and set(new) <= set(engine.EXPORTS)
    for name in new:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    for name in new[1:4]:
        assert engine._SIGNATURES[name] == engine._SIGNATURES["sg_window_node_trend"], name
    for name in new[7:]:
        assert engine._SIGNATURES[name] == engine._SIGNATURES["sg_window_nodes_top"], name
    assert all(callable(getattr(engine.ServiceGraph, m)) for m in METHODS)
    assert engine.ABI_VERSION == 6
    # no new structure class, no new *_DTYPE: every twin the module has is one tests/test_abi.py lays out
    twins = {n: v for n, v in vars(engine).items() if n.endswith("_DTYPE") or (isinstance(v, type) and issubclass(v, C.Structure) and n.startswith("Sg"))}
    assert not [n for n, v in twins.items() if not any(v is t for t in LAYOUTS.values())]
    assert engine.Q_SPACES == dict(nodes=1, groups=2, group_nodes=4) and engine.Q_MAX == 8
    assert engine.SEL_BY == dict(score=0, lat_dev=1, err_dev=2, new=3)
    assert engine.NSEL_BY == dict(score=0, in_lat_dev=1, in_err_dev=2, out_lat_dev=3, out_err_dev=4, new=5)


def test_set_quantile_trend(g):
    cfn = "sg_set_quantile_trend"
    g.set_quantile_trend()                                            # the node space, p99, every default
    g.set_quantile_trend(("nodes", "groups", "group_nodes"), 999, shift=2, ttl=9)
    g.set_quantile_trend("groups", 500, dict(warmup=1), max_entries=1 << 33)
    g.set_quantile_trend(6, 990, {})
    assert g._l.take() == [(cfn, "h", 1, 990, _packed()), (cfn, "h", 7, 999, _packed(shift=2, ttl=9)),
                           (cfn, "h", 2, 500, _packed(warmup=1, max_entries=1 << 33)), (cfn, "h", 6, 990, _packed())]
    g.set_quantile_trend(None)                                        # off: no spaces, or no parameters
    g.set_quantile_trend("nodes", 990, None)
    g.set_quantile_trend(params=None)
    assert g._l.take() == [(cfn, "h", 0, 990, _packed()), (cfn, "h", 1, 990, None), (cfn, "h", 1, 990, None)]
    with pytest.raises(TypeError) as ei:
        g.set_quantile_trend("nodes", 990, None, shift=3)
    assert str(ei.value) == "set_quantile_trend(params=None) switches the tail baselines off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_quantile_trend("nodes", 990, dict(zzz=1), aaa=2)
    assert str(ei.value) == "unknown tail trend parameters: ['aaa', 'zzz']"
    with pytest.raises(ValueError) as ei:
        g.set_quantile_trend(("nodes", "pods"))
    assert "unknown quantile space 'pods'" in str(ei.value) and g._l.take() == []
    text = b"sg_set_quantile_trend: the group percentiles are off (sg_set_quantiles, SG_Q_GROUPS)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_quantile_trend("groups")
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


READS = [("window_node_quantile_trend", "sg_window_node_quantile_trend", engine.NODE_TREND_DTYPE),
         ("window_group_quantile_trend", "sg_window_group_quantile_trend", engine.TREND_DTYPE),
         ("window_group_node_quantile_trend", "sg_window_group_node_quantile_trend", engine.NODE_TREND_DTYPE)]


@pytest.mark.parametrize("method,cfn,dtype", READS, ids=[r[0] for r in READS])
def test_indexed_reads(g, method, cfn, dtype):
    call = getattr(g, method)
    same(call(), dtype, pattern(dtype, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    a = call(index=None)
    same(a, dtype, pattern(dtype, 3))
    assert a.dtype == dtype
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    g._l.script[cfn] = dict(out=[2])
    same(call(index=[2, 0]), dtype, pattern(dtype, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    same(call(index=[]), dtype, pattern(dtype, 0))
    assert g._l.take() == []
    text = cfn.encode() + b": the last read window was closed while the node tail baseline was off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value).endswith(text.decode())


def test_buffer_entries_and_stats_take_one_space(g):
    cfn = "sg_window_quantile_trend_buffer"
    g._l.script = {cfn: dict(out=[0x3000])}
    assert g.window_quantile_trend_buffer("group_nodes") == 0x3000 == g.window_quantile_trend_buffer(1)
    assert g._l.take() == [(cfn, "h", 4, "out"), (cfn, "h", 1, "out")]
    cfn = "sg_quantile_trend_entries"
    g._l.script = {cfn: dict(out=[4])}
    e = g.quantile_trend_entries("groups")
    same(e, engine.TREND_ENTRY_DTYPE, pattern(engine.TREND_ENTRY_DTYPE, 4))
    assert e.dtype == engine.TREND_ENTRY_DTYPE
    assert g._l.take() == [(cfn, "h", 2, None, 0, "out"), (cfn, "h", 2, "buf", 4, "out")]
    cfn = "sg_quantile_trend_stats_get"
    g._l.script = {cfn: dict(fields=dict(entries=7, expired=1, dropped=2))}
    s = g.quantile_trend_stats("nodes")
    assert type(s) is engine.SgTrendStats and (s.entries, s.expired, s.dropped, s.windows) == (7, 1, 2, 0)
    assert g._l.take() == [(cfn, "h", 1, "out:SgTrendStats")]
    with pytest.raises(ValueError):
        g.quantile_trend_entries("edges")
    text = b"sg_quantile_trend_entries: space is one of SG_Q_NODES, SG_Q_GROUPS, SG_Q_GROUP_NODES"
    g._l.script = {"sg_quantile_trend_entries": dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.quantile_trend_entries(3)
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith(text.decode())


TOPS = [("window_nodes_top_tail", "sg_window_nodes_top_tail", engine.NODE_DTYPE, "sg_window_nodes", engine.NSEL_BY, "in_lat_dev"),
        ("window_group_nodes_top_tail", "sg_window_group_nodes_top_tail", engine.NODE_DTYPE, "sg_window_group_nodes", engine.NSEL_BY, "in_lat_dev"),
        ("window_groups_top_tail", "sg_window_groups_top_tail", engine.GROUP_EDGE_DTYPE, None, engine.SEL_BY, "lat_dev")]


@pytest.mark.parametrize("method,cfn,dtype,count,keys,default", TOPS, ids=[t[0] for t in TOPS])
def test_tail_selections(g, method, cfn, dtype, count, keys, default):
    call = getattr(g, method)
    g._l.script = {cfn: dict(out=[5, 6])}
    if count:
        g._l.script[count] = dict(out=[4])
    rows, idx, n = call(3, 0.5)                                       # cap = k; the default key is the tail's latency deviation
    assert g._l.take() == [(cfn, "h", keys[default], 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, dtype, pattern(dtype, 3)); same(idx, U4, pattern(U4, 3))
    assert rows.dtype == dtype and n == 6 and type(n) is int
    for by, b in keys.items():
        call(2, by=by, cap=9)
        assert g._l.take() == [(cfn, "h", b, 2, INF, "buf", "buf", 9, "out", "out")]
    rows, idx, n = call(0)                                            # k = 0: the window's row count (the group edges: max_edges)
    want_cap = 4 if count else 100
    calls = g._l.take()
    assert calls[-1] == (cfn, "h", keys[default], 0, INF, "buf", "buf", want_cap, "out", "out") and len(calls) == (2 if count else 1)
    with pytest.raises(ValueError):
        call(3, by="p99")
    text = cfn.encode() + b": the node tail baseline is off (sg_set_quantile_trend, SG_Q_NODES)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(1)
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()
