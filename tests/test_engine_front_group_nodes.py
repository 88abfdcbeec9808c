"""The front end's methods of the workload rows (K16) against the recording stand-in of tests/test_engine_front.py: the C calls they
make, what they return and the texts of their errors."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests.abi_layouts import LAYOUTS
from tests import engine_front as front

U4, same, pattern, INF = front.U4, front.same, front.pattern, front.INF
H, I, F, O, S, SO, Out = front.H, front.I, front.F, front.O, front.S, front.SO, front.Out
NEW_ABI = {
    "sg_set_group_nodes": [H, I], "sg_set_group_node_trend": [H, S],
    "sg_window_group_nodes": front._COUNTED(engine.NODE_DTYPE), "sg_window_group_nodes_buffer": [H, O, O],
    "sg_window_group_node_trend": front._INDEXED(engine.NODE_TREND_DTYPE), "sg_window_group_node_trend_buffer": [H, O],
    "sg_group_node_trend_entries": front._COUNTED(engine.TREND_ENTRY_DTYPE), "sg_group_node_trend_stats_get": [H, SO],
    "sg_window_group_nodes_top": [H, I, I, F, Out(engine.NODE_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_group_nodes_select": [H, I, I, F, I, I, I, I, I],
}
_TREND = [("shift", 4), ("warmup", 4), ("ttl", 64), ("max_entries", 0), ("lat_floor_ns", 1000), ("err_floor", 10486)]


g = front.abi_fixture(NEW_ABI)


def _trend_bytes(**over):
    v = [over.get("struct_size", 40)] + [over.get(f, d) for f, d in _TREND] + [over.get("reserved", 0)]
    return struct.pack("<4I2Q2I", *v)


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 10
    for name, kinds in NEW_ABI.items():
        assert len(engine._SIGNATURES[name][1]) == len(kinds), name
    assert engine._SIGNATURES["sg_set_group_nodes"][1][1] is C.c_int


def test_set_group_nodes(g):
    assert g.set_group_nodes() is None and g.set_group_nodes(False) is None and g.set_group_nodes(on=True) is None
    assert g._l.take() == [("sg_set_group_nodes", "h", 1), ("sg_set_group_nodes", "h", 0), ("sg_set_group_nodes", "h", 1)]
    text = b"sg_set_group_nodes: max_groups + the node capacity exceeds 2^21 group keys: pass a tighter max_groups to sg_set_groups"
    g._l.script = {"sg_set_group_nodes": dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_nodes()
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value) == "servicegraph rc=-22: " + text.decode()
    g._l.script = {"sg_set_group_nodes": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"sg_set_group_nodes: the groups are off (sg_set_groups)")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_nodes()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: sg_set_group_nodes: the groups are off (sg_set_groups)"


def test_set_group_node_trend(g):
    assert g.set_group_node_trend() is None and g.set_group_node_trend(dict(shift=2), ttl=9) is None and g.set_group_node_trend(None) is None
    assert g._l.take() == [("sg_set_group_node_trend", "h", _trend_bytes()), ("sg_set_group_node_trend", "h", _trend_bytes(shift=2, ttl=9)),
                           ("sg_set_group_node_trend", "h", None)]
    with pytest.raises(TypeError) as ei:
        g.set_group_node_trend(None, shift=1)
    assert str(ei.value) == "set_group_node_trend(None) switches the workload trend off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_node_trend(zzz=1)
    assert str(ei.value) == "unknown workload trend parameters: ['zzz']"
    assert g._l.take() == []
    text = b"sg_set_group_node_trend: the workload rows are off (sg_set_group_nodes)"
    g._l.script = {"sg_set_group_node_trend": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_node_trend()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_nodes_is_a_counted_readback(g):
    cfn, dt = "sg_window_group_nodes", engine.NODE_DTYPE
    same(g.window_group_nodes(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_nodes(), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, "out"), (cfn, "h", "buf", 3, "out")]
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"sg_window_group_nodes: the workload rows are off (sg_set_group_nodes)")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_nodes()
    assert str(ei.value) == "servicegraph rc=-71: sg_window_group_nodes: the workload rows are off (sg_set_group_nodes)"


def test_window_group_node_trend_is_an_indexed_readback(g):
    cfn, dt = "sg_window_group_node_trend", engine.NODE_TREND_DTYPE
    same(g.window_group_node_trend(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_node_trend(index=None), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(g.window_group_node_trend(index=[]), dt, pattern(dt, 0))
    assert g._l.take() == []
    g._l.script[cfn] = dict(out=[2])
    same(g.window_group_node_trend([2, 0]), dt, pattern(dt, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]


def test_entries_stats_and_buffers(g):
    g._l.script = {"sg_group_node_trend_entries": dict(out=[3]), "sg_group_node_trend_stats_get": dict(fields=dict(windows=4, dropped=2)),
                   "sg_window_group_node_trend_buffer": dict(out=[0x1000]), "sg_window_group_nodes_buffer": dict(out=[0x2000, 0x3000])}
    same(g.group_node_trend_entries(), engine.TREND_ENTRY_DTYPE, pattern(engine.TREND_ENTRY_DTYPE, 3))
    s = g.group_node_trend_stats()
    assert type(s) is engine.SgTrendStats and (s.windows, s.entries, s.dropped) == (4, 0, 2)
    assert g.window_group_node_trend_buffer() == 0x1000 and g.window_group_nodes_buffer() == (0x2000, 0x3000)
    assert g._l.take() == [("sg_group_node_trend_entries", "h", None, 0, "out"), ("sg_group_node_trend_entries", "h", "buf", 3, "out"),
                           ("sg_group_node_trend_stats_get", "h", "out:SgTrendStats"), ("sg_window_group_node_trend_buffer", "h", "out"),
                           ("sg_window_group_nodes_buffer", "h", "out", "out")]
    g._l.script = {"sg_window_group_nodes_buffer": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_nodes_buffer()
    assert str(ei.value) == "servicegraph rc=-71: off"


def test_window_group_nodes_top_and_select(g):
    cfn = "sg_window_group_nodes_top"
    g._l.script = {cfn: dict(out=[5, 6]), "sg_window_group_nodes": dict(out=[4]), "sg_window_nodes": dict(out=[99])}
    rows, idx, n = g.window_group_nodes_top(3, 0.5, by="in_err_dev")  # cap = k: 5 selected, 3 fit
    assert g._l.take() == [(cfn, "h", 2, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, engine.NODE_DTYPE, pattern(engine.NODE_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 6 and type(n) is int
    rows, idx, n = g.window_group_nodes_top(0)                        # k = 0, cap=None: the window's workload rows, not its node rows
    assert g._l.take() == [("sg_window_group_nodes", "h", None, 0, "out"), (cfn, "h", 0, 0, INF, "buf", "buf", 4, "out", "out")]
    assert len(rows) == len(idx) == 4
    rows, idx, n = g.window_group_nodes_top(0, cap=9, by="new")
    assert g._l.take() == [(cfn, "h", 5, 0, INF, "buf", "buf", 9, "out", "out")]
    assert len(rows) == len(idx) == 5
    for bad in ("x", 2, "lat_dev"):                                   # SG_NSEL_*'s names, never a number or an edge key
        with pytest.raises(ValueError) as ei:
            g.window_group_nodes_top(3, by=bad)
        assert str(ei.value) == f"by must be one of {sorted(engine.NSEL_BY)}, not {bad!r}"
    assert g._l.take() == []
    text = b"workload selection by a trend key: the workload trend is off (sg_set_group_node_trend)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_nodes_top(3, by="out_lat_dev")
    assert str(ei.value) == "servicegraph rc=-71: " + text.decode()
    g._l.take()
    assert g.window_group_nodes_select(3, 0.5, 0x1000, 0x2000, 8, 0x3000, stream=0x4000) is None
    assert g.window_group_nodes_select(0, 1.5, 0, 0x2000, 8, 0x3000, by="out_lat_dev") is None
    assert g._l.take() == [("sg_window_group_nodes_select", "h", 0, 3, 0.5, 0x1000, 0x2000, 8, 0x3000, 0x4000),
                           ("sg_window_group_nodes_select", "h", 3, 0, 1.5, None, 0x2000, 8, 0x3000, None)]


def test_window_nodes_top_still_counts_the_node_rows(g):
    g._l.script = {"sg_window_nodes_top": dict(out=[2, 7]), "sg_window_nodes": dict(out=[7]), "sg_window_group_nodes": dict(out=[3])}
    g.window_nodes_top(0)
    assert g._l.take() == [("sg_window_nodes", "h", None, 0, "out"), ("sg_window_nodes_top", "h", 0, 0, INF, "buf", "buf", 7, "out", "out")]


def test_the_stage_adds_no_struct_and_no_constant_set():
    twins = {n: v for n, v in vars(engine).items() if (n.startswith("Sg") and isinstance(v, type) and issubclass(v, C.Structure))
             or (n.endswith("_DTYPE") and isinstance(v, np.dtype))}
    assert all(any(v is t for t in LAYOUTS.values()) for v in twins.values()) and len(twins) == len(LAYOUTS) == 23
    assert engine.NSEL_BY == dict(score=0, in_lat_dev=1, in_err_dev=2, out_lat_dev=3, out_err_dev=4, new=5) and engine.ABI_VERSION == 6
    st = engine._STAGES
    assert st["group_node_trend"].struct is st["node_trend"].struct is engine.SgTrendParams
    assert st["group_node_trend"].defaults is engine.TREND_DEFAULTS
