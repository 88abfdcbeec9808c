"""The front end's methods of the workload ranking (K17) against the recording stand-in of tests/test_engine_front.py: the C calls
they make, what they return and the texts of their errors."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests.abi_layouts import LAYOUTS
from tests import engine_front as front

U4, same, pattern, INF = front.U4, front.same, front.pattern, front.INF
H, I, F, O, S, Out = front.H, front.I, front.F, front.O, front.S, front.Out
NEW_ABI = {
    "sg_set_group_rank": [H, S], "sg_window_group_rank": front._INDEXED(engine.RANK_DTYPE), "sg_window_group_rank_buffer": [H, O],
    "sg_window_group_rank_top": [H, I, F, Out(engine.NODE_DTYPE, 6), Out(engine.RANK_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_group_rank_select": [H, I, F, I, I, I, I, I],
    "sg_window_group_nodes": front._COUNTED(engine.NODE_DTYPE),        # (the count behind a k = 0 selection)
}
_RANK = [("iters", 0), ("damping_q8", 0), ("seed", 0), ("seed_min_score", 0.0)]


g = front.abi_fixture(NEW_ABI)


def _rank_bytes(**over):
    v = [over.get("struct_size", 24)] + [over.get(f, d) for f, d in _RANK] + [over.get("reserved", 0)]
    return struct.pack("<4IfI", *v)


def test_the_new_c_functions_are_in_the_signature_table():
    new = [n for n in NEW_ABI if "rank" in n]
    assert set(new) <= set(engine.EXPORTS) and len(new) == 5
    for name in new:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
        assert engine._SIGNATURES[name] == engine._SIGNATURES[name.replace("group_", "")], name    # K11's shapes, call for call


def test_set_group_rank(g):
    assert g.set_group_rank() is None and g.set_group_rank(dict(iters=5), seed_min_score=0.25) is None and g.set_group_rank(None) is None
    assert g.set_group_rank(seed="uniform") is None and g.set_group_rank(seed=1, struct_size=8, reserved=7) is None
    assert g._l.take() == [("sg_set_group_rank", "h", _rank_bytes()), ("sg_set_group_rank", "h", _rank_bytes(iters=5, seed_min_score=0.25)),
                           ("sg_set_group_rank", "h", None), ("sg_set_group_rank", "h", _rank_bytes(seed=1)),
                           ("sg_set_group_rank", "h", _rank_bytes(seed=1, struct_size=8, reserved=7))]
    with pytest.raises(TypeError) as ei:
        g.set_group_rank(None, iters=1)
    assert str(ei.value) == "set_group_rank(None) switches the workload ranking off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_rank(zzz=1)
    assert str(ei.value) == "unknown workload rank parameters: ['zzz']"
    with pytest.raises(ValueError) as ei:
        g.set_group_rank(seed="x")
    assert str(ei.value) == "seed must be one of ['score', 'uniform'], not 'x'"
    assert g._l.take() == []
    text = b"sg_set_group_rank: the workload rows are off (sg_set_group_nodes)"
    g._l.script = {"sg_set_group_rank": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_rank()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_rank_is_an_indexed_readback(g):
    cfn, dt = "sg_window_group_rank", engine.RANK_DTYPE
    same(g.window_group_rank(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_rank(index=None), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(g.window_group_rank(index=[]), dt, pattern(dt, 0))
    assert g._l.take() == []
    g._l.script[cfn] = dict(out=[2])
    same(g.window_group_rank([2, 0]), dt, pattern(dt, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    text = b"sg_window_group_rank: the last read window was closed while the workload ranking was off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_rank()
    assert str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_rank_buffer(g):
    g._l.script = {"sg_window_group_rank_buffer": dict(out=[0x1000])}
    assert g.window_group_rank_buffer() == 0x1000
    assert g._l.take() == [("sg_window_group_rank_buffer", "h", "out")]
    g._l.script = {"sg_window_group_rank_buffer": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_rank_buffer()
    assert str(ei.value) == "servicegraph rc=-71: off"


def test_window_group_rank_top_and_select(g):
    cfn = "sg_window_group_rank_top"
    g._l.script = {cfn: dict(out=[5, 6]), "sg_window_group_nodes": dict(out=[4]), "sg_window_nodes": dict(out=[99])}
    rows, rk, idx, n = g.window_group_rank_top(3, 0.25)               # cap = k: 5 selected, 3 fit
    assert g._l.take() == [(cfn, "h", 3, 0.25, "buf", "buf", "buf", 3, "out", "out")]
    same(rows, engine.NODE_DTYPE, pattern(engine.NODE_DTYPE, 3))
    same(rk, engine.RANK_DTYPE, pattern(engine.RANK_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 6 and type(n) is int
    rows, rk, idx, n = g.window_group_rank_top(0)                     # k = 0, cap=None: the window's workload rows, not its node rows
    assert g._l.take() == [("sg_window_group_nodes", "h", None, 0, "out"), (cfn, "h", 0, INF, "buf", "buf", "buf", 4, "out", "out")]
    assert len(rows) == len(rk) == len(idx) == 4
    rows, rk, idx, n = g.window_group_rank_top(2, cap=9)
    assert g._l.take() == [(cfn, "h", 2, INF, "buf", "buf", "buf", 9, "out", "out")]
    assert len(rows) == len(rk) == len(idx) == 5
    text = b"workload rank selection: the workload ranking is off (sg_set_group_rank)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_rank_top(3)
    assert str(ei.value) == "servicegraph rc=-71: " + text.decode()
    g._l.take()
    assert g.window_group_rank_select(3, 0.5, 0x1000, 0x2000, 8, 0x3000, stream=0x4000) is None
    assert g.window_group_rank_select(0, 1.5, 0, 0x2000, 8, 0x3000) is None
    assert g._l.take() == [("sg_window_group_rank_select", "h", 3, 0.5, 0x1000, 0x2000, 8, 0x3000, 0x4000),
                           ("sg_window_group_rank_select", "h", 0, 1.5, None, 0x2000, 8, 0x3000, None)]


def test_window_rank_top_still_counts_the_node_rows(g):
    g._l.script = {"sg_window_rank_top": dict(out=[2, 7]), "sg_window_nodes": dict(out=[7]), "sg_window_group_nodes": dict(out=[3])}
    g.window_rank_top(0)
    assert g._l.take() == [("sg_window_nodes", "h", None, 0, "out"), ("sg_window_rank_top", "h", 0, INF, "buf", "buf", "buf", 7, "out", "out")]


def test_the_stage_adds_no_struct_and_no_constant():
    twins = {n: v for n, v in vars(engine).items() if (n.startswith("Sg") and isinstance(v, type) and issubclass(v, C.Structure))
             or (n.endswith("_DTYPE") and isinstance(v, np.dtype))}
    assert all(any(v is t for t in LAYOUTS.values()) for v in twins.values()) and len(twins) == len(LAYOUTS) == 23
    assert engine.RANK_SEED == dict(score=0, uniform=1) and engine.ABI_VERSION == 6
    st = engine._STAGES
    assert st["group_rank"].struct is st["rank"].struct is engine.SgRankParams
    assert st["group_rank"].defaults is st["rank"].defaults is engine.RANK_DEFAULTS and st["group_rank"].convert is not None
