"""The front end's methods of the SLO burn rates (K24) against the recording stand-in of tests/engine_front.py: the C calls they make
(argument order, buffers inside numpy arrays), the dtypes they return, the texts of their errors, and what the stage adds to the
module: nine functions, two structs, the constant sets."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern = front.same, front.pattern
H, I, O, S, SO, U4, Out, In = front.H, front.I, front.O, front.S, front.SO, front.U4, front.Out, front.In
ROW = np.dtype(("<u8", (engine.SLO_WORDS,)))
ENTRY = np.dtype(("<u8", (engine.SLO_ENTRY_WORDS,)))
TOP = [H, I, I, I, Out(engine.NODE_DTYPE, 6), Out(U4, 6), I, O, O]   # f(h, by, k, min_value_q10, out, index, cap, *n_selected, *n_rows)
NEW_ABI = {
    "sg_set_slo": [H, I, S],
    "sg_slo_assign": [H, I, In(U4, 4), In(U4, 4), I],
    "sg_window_node_slo": front._INDEXED(ROW), "sg_window_group_node_slo": front._INDEXED(ROW),
    "sg_window_slo_buffer": [H, I, O],
    "sg_slo_entries": [H, I, Out(ENTRY, 3), I, O],
    "sg_slo_stats_get": [H, I, SO],
    "sg_window_nodes_top_slo": TOP, "sg_window_group_nodes_top_slo": TOP,
    "sg_window_group_nodes": front._COUNTED(engine.NODE_DTYPE),
}
METHODS = ("set_slo", "slo_assign", "window_node_slo", "window_group_node_slo", "window_slo_buffer", "slo_entries", "slo_stats",
           "window_nodes_top_slo", "window_group_nodes_top_slo")
_FIELDS = [("latency_bin", 10), ("latency_target_ppm", 990_000), ("error_target_ppm", 999_000), ("short_windows", 2), ("long_windows", 12),
           ("min_burn_q10", 14746)]


def _packed(**over):
    return struct.pack("<8IQ", 40, *[over.get(f, d) for f, d in _FIELDS], over.get("reserved", 0), over.get("min_requests", 100))


g = front.abi_fixture(NEW_ABI)


def test_nine_functions_two_structs_and_the_constants():
    new = [n for n in NEW_ABI if n != "sg_window_group_nodes"]
    assert len(new) == 9 and set(new) <= set(engine.EXPORTS)
    for name in new:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    assert engine._SIGNATURES["sg_window_node_slo"] == engine._SIGNATURES["sg_window_group_node_slo"] == engine._SIGNATURES["sg_window_group_node_hops"]
    assert engine._SIGNATURES["sg_window_nodes_top_slo"] == engine._SIGNATURES["sg_window_group_nodes_top_slo"]
    assert all(callable(getattr(engine.ServiceGraph, m)) for m in METHODS)
    assert engine.ABI_VERSION == 6                                    # additive: the version does not move
    assert C.sizeof(engine.SloParams) == 40 == len(_packed()) and C.sizeof(engine.SloStats) == 32
    assert engine.SLO_DEFAULTS == dict(_FIELDS, min_requests=100)
    assert (engine.SLO_WORDS, engine.SLO_ENTRY_WORDS, engine.SLO_MAX_WINDOWS, len(engine.SLO_SIDE_FIELDS)) == (18, 14, 64, 8)
    assert engine.SLOSEL_BY == dict(err=0, slow=1) and engine.SLOSEL_SIDE == {"in": 2, "out": 4}


def test_set_slo(g):
    cfn = "sg_set_slo"
    g.set_slo()                                                       # the workload space, every default
    g.set_slo(("nodes", "group_nodes"), latency_bin=3, long_windows=64, min_requests=1 << 40)
    g.set_slo("nodes", dict(short_windows=1), min_burn_q10=1024)
    g.set_slo(5, {})
    assert g._l.take() == [(cfn, "h", 4, _packed()), (cfn, "h", 5, _packed(latency_bin=3, long_windows=64, min_requests=1 << 40)),
                           (cfn, "h", 1, _packed(short_windows=1, min_burn_q10=1024)), (cfn, "h", 5, _packed())]
    g.set_slo(None)                                                   # off: no spaces, or no parameters
    g.set_slo("nodes", None)
    g.set_slo(params=None)
    assert g._l.take() == [(cfn, "h", 0, _packed()), (cfn, "h", 1, None), (cfn, "h", 4, None)]
    with pytest.raises(TypeError) as ei:
        g.set_slo("nodes", None, latency_bin=3)
    assert str(ei.value) == "set_slo(params=None) switches the SLO stage off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_slo("nodes", dict(zzz=1), shift=2)
    assert str(ei.value) == "unknown SLO parameters: ['shift', 'zzz']"
    with pytest.raises(ValueError):
        g.set_slo(("nodes", "edges"))
    assert g._l.take() == []
    text = b"sg_set_slo: the workload percentiles are off (sg_set_quantiles, SG_Q_GROUP_NODES)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_slo()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_slo_assign(g):
    cfn = "sg_slo_assign"
    word = engine.slo_objective(2, 999_000, 999_900)
    g.slo_assign("group_nodes", [3 << 30 | 7, 21], [word, 0])
    g.slo_assign(1, np.array([5], np.uint64), (word,))
    g.slo_assign("nodes", [], [])
    assert g._l.take() == [(cfn, "h", 4, ("in", [3 << 30 | 7, 21]), ("in", [word, 0]), 2), (cfn, "h", 1, ("in", [5]), ("in", [word]), 1),
                           (cfn, "h", 1, ("in", []), ("in", []), 0)]
    with pytest.raises(ValueError):
        g.slo_assign("nodes", [1, 2], [0])
    assert g._l.take() == []


READS = [("window_node_slo", "sg_window_node_slo"), ("window_group_node_slo", "sg_window_group_node_slo")]


@pytest.mark.parametrize("method,cfn", READS, ids=[r[0] for r in READS])
def test_indexed_reads(g, method, cfn):
    call = getattr(g, method)
    same(call(), ROW, pattern(ROW, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    a = call(index=None)
    same(a, ROW, pattern(ROW, 3))
    assert a.shape == (3, 18) and a.dtype == np.dtype("<u8")
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    g._l.script[cfn] = dict(out=[2])
    same(call(index=[2, 0]), ROW, pattern(ROW, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    text = cfn.encode() + b": the last read window was closed while the node SLO stage was off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value).endswith(text.decode())


def test_buffer_entries_and_stats_take_one_space(g):
    cfn = "sg_window_slo_buffer"
    g._l.script = {cfn: dict(out=[0x3000])}
    assert g.window_slo_buffer("group_nodes") == 0x3000 == g.window_slo_buffer(1)
    assert g._l.take() == [(cfn, "h", 4, "out"), (cfn, "h", 1, "out")]
    cfn = "sg_slo_entries"
    g._l.script = {cfn: dict(out=[4])}
    e = g.slo_entries("nodes")
    same(e, ENTRY, pattern(ENTRY, 4))
    assert e.shape == (4, 14)
    assert g._l.take() == [(cfn, "h", 1, None, 0, "out"), (cfn, "h", 1, "buf", 4, "out")]
    cfn = "sg_slo_stats_get"
    g._l.script = {cfn: dict(fields=dict(windows=9, keys_active=7, sides_burning=2, keys=316))}
    s = g.slo_stats("group_nodes")
    assert type(s) is engine.SloStats and (s.windows, s.keys_active, s.sides_burning, s.keys) == (9, 7, 2, 316)
    assert g._l.take() == [(cfn, "h", 4, "out:SloStats")]
    with pytest.raises(ValueError):
        g.slo_entries("pods")
    text = b"sg_slo_entries: space is SG_Q_NODES or SG_Q_GROUP_NODES"
    g._l.script = {"sg_slo_entries": dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.slo_entries(2)
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith(text.decode())


TOPS = [("window_nodes_top_slo", "sg_window_nodes_top_slo", "sg_window_nodes"),
        ("window_group_nodes_top_slo", "sg_window_group_nodes_top_slo", "sg_window_group_nodes")]


@pytest.mark.parametrize("method,cfn,count", TOPS, ids=[t[0] for t in TOPS])
def test_slo_selections(g, method, cfn, count):
    call, dtype = getattr(g, method), engine.NODE_DTYPE
    g._l.script = {cfn: dict(out=[5, 6]), count: dict(out=[4])}
    rows, idx, n = call(3, 1024)                                      # cap = k; the default key: the errors of the in side
    assert g._l.take() == [(cfn, "h", 0 | 2, 3, 1024, "buf", "buf", 3, "out", "out")]
    same(rows, dtype, pattern(dtype, 3)); same(idx, U4, pattern(U4, 3))
    assert rows.dtype == dtype and n == 6 and type(n) is int
    for by, b in engine.SLOSEL_BY.items():
        for side, sb in engine.SLOSEL_SIDE.items():
            call(2, by=by, side=side, cap=9)
            assert g._l.take() == [(cfn, "h", b | sb, 2, 0, "buf", "buf", 9, "out", "out")]
    call(2, by=5, cap=9)                                              # the SG_SLOSEL_* int as it is
    assert g._l.take() == [(cfn, "h", 5, 2, 0, "buf", "buf", 9, "out", "out")]
    call(0)                                                           # k = 0: the window's row count
    calls = g._l.take()
    assert calls[-1] == (cfn, "h", 2, 0, 0, "buf", "buf", 4, "out", "out") and len(calls) == 2
    with pytest.raises(ValueError):
        call(3, by="p99")
    with pytest.raises(ValueError):
        call(3, by="err", side="both")
    text = cfn.encode() + b": the node SLO stage is off (sg_set_slo, SG_Q_NODES)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(1)
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()
