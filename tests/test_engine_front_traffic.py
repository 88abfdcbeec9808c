"""The front end's methods of the traffic baselines (K23) against the recording stand-in of tests/test_engine_front.py: the C calls
they make (argument order, buffers inside numpy arrays), the dtypes they return, the texts of their errors, and what the stage adds
to the module: eleven functions, one parameter struct, three constant sets."""
import ctypes as C
import struct

import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern, INF = front.same, front.pattern, front.INF
H, I, F, O, S, SO, U4, Out = front.H, front.I, front.F, front.O, front.S, front.SO, front.U4, front.Out
TOP = lambda dt: [H, I, I, F, Out(dt, 6), Out(U4, 6), I, O, O]     # f(h, by, k, min_value, out, index, cap, *n_selected, *n_rows)
NEW_ABI = {
    "sg_set_traffic_trend": [H, I, S],
    "sg_window_traffic": front._INDEXED(engine.TREND_DTYPE),
    "sg_window_node_traffic": front._INDEXED(engine.NODE_TREND_DTYPE),
    "sg_window_group_traffic": front._INDEXED(engine.TREND_DTYPE),
    "sg_window_group_node_traffic": front._INDEXED(engine.NODE_TREND_DTYPE),
    "sg_window_traffic_buffer": [H, I, O],
    "sg_traffic_trend_entries": [H, I, Out(engine.TREND_ENTRY_DTYPE, 3), I, O],
    "sg_traffic_trend_stats_get": [H, I, SO],
    "sg_window_nodes_top_traffic": TOP(engine.NODE_DTYPE), "sg_window_groups_top_traffic": TOP(engine.GROUP_EDGE_DTYPE),
    "sg_window_group_nodes_top_traffic": TOP(engine.NODE_DTYPE),
    "sg_window_group_nodes": front._COUNTED(engine.NODE_DTYPE),
}
METHODS = ("set_traffic_trend", "window_traffic", "window_node_traffic", "window_group_traffic", "window_group_node_traffic",
           "window_traffic_buffer", "traffic_trend_entries", "traffic_trend_stats", "window_nodes_top_traffic", "window_groups_top_traffic",
           "window_group_nodes_top_traffic")
_FIELDS = [("shift", 4), ("warmup", 4), ("ttl", 64), ("max_entries", 0), ("load_floor_ns", 1_000_000), ("rate_floor", 8)]


def _packed(**over):
    return struct.pack("<4I2Q2I", 40, *[over.get(f, d) for f, d in _FIELDS], 0)


g = front.abi_fixture(NEW_ABI)


def test_eleven_functions_one_struct_three_constant_sets():
    new = [n for n in NEW_ABI if n != "sg_window_group_nodes"]
    assert len(new) == 11 and set(new) <= set(engine.EXPORTS)
    for name in new:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    for name in new[1:5]:
        assert engine._SIGNATURES[name] == engine._SIGNATURES["sg_window_node_trend"], name
    for name in new[8:]:
        assert engine._SIGNATURES[name] == engine._SIGNATURES["sg_window_nodes_top_tail"], name
    assert all(callable(getattr(engine.ServiceGraph, m)) for m in METHODS)
    assert engine.ABI_VERSION == 6                                    # additive: the version does not move
    assert engine.T_SPACES == dict(edges=1, nodes=2, groups=4, group_nodes=8)
    assert engine.TSEL_BY == dict(surge=0, drop=1, load_up=2, load_down=3) and engine.TSEL_SIDE == {"in": 4, "out": 8}
    assert C.sizeof(engine.TrafficParams) == 40 == len(_packed())
    assert engine.TRAFFIC_DEFAULTS == dict(_FIELDS)


def test_set_traffic_trend(g):
    cfn = "sg_set_traffic_trend"
    g.set_traffic_trend()                                             # the node space, every default
    g.set_traffic_trend(("edges", "nodes", "groups", "group_nodes"), shift=2, ttl=9, rate_floor=3)
    g.set_traffic_trend("groups", dict(warmup=1), load_floor_ns=1 << 52, max_entries=1 << 33)
    g.set_traffic_trend(9, {})
    assert g._l.take() == [(cfn, "h", 2, _packed()), (cfn, "h", 15, _packed(shift=2, ttl=9, rate_floor=3)),
                           (cfn, "h", 4, _packed(warmup=1, load_floor_ns=1 << 52, max_entries=1 << 33)), (cfn, "h", 9, _packed())]
    g.set_traffic_trend(None)                                         # off: no spaces, or no parameters
    g.set_traffic_trend("nodes", None)
    g.set_traffic_trend(params=None)
    assert g._l.take() == [(cfn, "h", 0, _packed()), (cfn, "h", 2, None), (cfn, "h", 2, None)]
    with pytest.raises(TypeError) as ei:
        g.set_traffic_trend("nodes", None, shift=3)
    assert str(ei.value) == "set_traffic_trend(params=None) switches the traffic baselines off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_traffic_trend("nodes", dict(zzz=1), lat_floor_ns=2)
    assert str(ei.value) == "unknown traffic trend parameters: ['lat_floor_ns', 'zzz']"
    with pytest.raises(ValueError) as ei:
        g.set_traffic_trend(("nodes", "pods"))
    assert "unknown traffic space 'pods'" in str(ei.value) and g._l.take() == []
    text = b"sg_set_traffic_trend: the groups are off (sg_set_groups)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_traffic_trend("groups")
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


READS = [("window_traffic", "sg_window_traffic", engine.TREND_DTYPE), ("window_node_traffic", "sg_window_node_traffic", engine.NODE_TREND_DTYPE),
         ("window_group_traffic", "sg_window_group_traffic", engine.TREND_DTYPE),
         ("window_group_node_traffic", "sg_window_group_node_traffic", engine.NODE_TREND_DTYPE)]


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
    text = cfn.encode() + b": the last read window was closed while the node traffic baseline was off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value).endswith(text.decode())


def test_buffer_entries_and_stats_take_one_space(g):
    cfn = "sg_window_traffic_buffer"
    g._l.script = {cfn: dict(out=[0x3000])}
    assert g.window_traffic_buffer("group_nodes") == 0x3000 == g.window_traffic_buffer(1)
    assert g._l.take() == [(cfn, "h", 8, "out"), (cfn, "h", 1, "out")]
    cfn = "sg_traffic_trend_entries"
    g._l.script = {cfn: dict(out=[4])}
    e = g.traffic_trend_entries("groups")
    same(e, engine.TREND_ENTRY_DTYPE, pattern(engine.TREND_ENTRY_DTYPE, 4))
    assert e.dtype == engine.TREND_ENTRY_DTYPE
    assert g._l.take() == [(cfn, "h", 4, None, 0, "out"), (cfn, "h", 4, "buf", 4, "out")]
    cfn = "sg_traffic_trend_stats_get"
    g._l.script = {cfn: dict(fields=dict(entries=7, expired=1, dropped=2))}
    s = g.traffic_trend_stats("edges")
    assert type(s) is engine.SgTrendStats and (s.entries, s.expired, s.dropped, s.windows) == (7, 1, 2, 0)
    assert g._l.take() == [(cfn, "h", 1, "out:SgTrendStats")]
    with pytest.raises(ValueError):
        g.traffic_trend_entries("pods")
    text = b"sg_traffic_trend_entries: space is one of SG_T_EDGES, SG_T_NODES, SG_T_GROUPS, SG_T_GROUP_NODES"
    g._l.script = {"sg_traffic_trend_entries": dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.traffic_trend_entries(3)
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith(text.decode())


TOPS = [("window_nodes_top_traffic", "sg_window_nodes_top_traffic", engine.NODE_DTYPE, "sg_window_nodes", True),
        ("window_group_nodes_top_traffic", "sg_window_group_nodes_top_traffic", engine.NODE_DTYPE, "sg_window_group_nodes", True),
        ("window_groups_top_traffic", "sg_window_groups_top_traffic", engine.GROUP_EDGE_DTYPE, None, False)]


@pytest.mark.parametrize("method,cfn,dtype,count,sided", TOPS, ids=[t[0] for t in TOPS])
def test_traffic_selections(g, method, cfn, dtype, count, sided):
    call = getattr(g, method)
    g._l.script = {cfn: dict(out=[5, 6])}
    if count:
        g._l.script[count] = dict(out=[4])
    default = 1 | 4 if sided else 1                                   # the default key: the drop (of the in side)
    rows, idx, n = call(3, 0.5)                                       # cap = k
    assert g._l.take() == [(cfn, "h", default, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, dtype, pattern(dtype, 3)); same(idx, U4, pattern(U4, 3))
    assert rows.dtype == dtype and n == 6 and type(n) is int
    for by, b in engine.TSEL_BY.items():
        for side, sb in (engine.TSEL_SIDE.items() if sided else [(None, 0)]):
            call(2, by=by, cap=9, **(dict(side=side) if sided else {}))
            assert g._l.take() == [(cfn, "h", b | sb, 2, INF, "buf", "buf", 9, "out", "out")]
    call(2, by=11, cap=9)                                             # the SG_TSEL_* int as it is
    assert g._l.take() == [(cfn, "h", 11, 2, INF, "buf", "buf", 9, "out", "out")]
    rows, idx, n = call(0)                                            # k = 0: the window's row count (the group edges: max_edges)
    want_cap = 4 if count else 100
    calls = g._l.take()
    assert calls[-1] == (cfn, "h", default, 0, INF, "buf", "buf", want_cap, "out", "out") and len(calls) == (2 if count else 1)
    with pytest.raises(ValueError):
        call(3, by="p99")
    if sided:
        with pytest.raises(ValueError):
            call(3, by="drop", side="both")
    text = cfn.encode() + b": the node traffic baseline is off (sg_set_traffic_trend, SG_T_NODES)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(1)
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()
