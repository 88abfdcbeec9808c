"""The front end's methods of the replica outliers (K25) against the recording stand-in of tests/engine_front.py: the C calls they make
(argument order, buffers inside numpy arrays), the dtypes they return, the texts of their errors, and what the stage adds to the
module: five functions, one struct, the constant sets.  set_replicas is sg_set_replicas' front end."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern = front.same, front.pattern
H, I, O, S, U4, Out = front.H, front.I, front.O, front.S, front.U4, front.Out
ROW = np.dtype(("<u4", (engine.REPLICA_WORDS,)))
GROUP_ROW = np.dtype(("<u4", (engine.REPLICA_GROUP_WORDS,)))
NEW_ABI = {
    "sg_set_replicas": [H, S],
    "sg_window_replicas": front._INDEXED(ROW), "sg_window_group_replicas": front._INDEXED(GROUP_ROW),
    "sg_window_replicas_buffer": [H, O, O],
    "sg_window_replicas_top": [H, I, I, I, Out(engine.NODE_DTYPE, 6), Out(U4, 6), I, O, O],   # f(h, by, k, min_value, out, index, cap, *n_selected, *n_rows)
    "sg_window_nodes": front._COUNTED(engine.NODE_DTYPE),
}
METHODS = ("set_replicas", "window_replicas", "window_group_replicas", "window_replicas_buffer", "window_replicas_top")
_FIELDS = ("min_replicas", "min_requests", "min_err_excess_q20", "min_lat_ratio_q10", "tail_permille", "min_tail_bins")


def _packed(**over):
    return struct.pack("<2IQ6I", 40, *[over.get(f, 0) for f in _FIELDS], *over.get("reserved", (0, 0)))


g = front.abi_fixture(NEW_ABI)


def test_five_functions_one_struct_and_the_constants():
    new = [n for n in NEW_ABI if n != "sg_window_nodes"]
    assert len(new) == 5 and set(new) <= set(engine.EXPORTS)
    for name in new:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    assert engine._SIGNATURES["sg_window_replicas"] == engine._SIGNATURES["sg_window_group_replicas"] == engine._SIGNATURES["sg_window_node_slo"]
    assert engine._SIGNATURES["sg_window_replicas_top"] == engine._SIGNATURES["sg_window_nodes_top_slo"]
    assert all(callable(getattr(engine.ServiceGraph, m)) for m in METHODS)
    assert engine.ABI_VERSION == 6                                    # additive: the version does not move
    assert C.sizeof(engine.ReplicaParams) == 40 == len(_packed())
    assert engine.REPLICA_DEFAULTS == dict.fromkeys(_FIELDS, 0)       # a 0 is the stage's own default
    assert (engine.REPLICA_WORDS, engine.REPLICA_GROUP_WORDS) == (12, 8) == (2 + 2 * len(engine.REPLICA_SIDE_FIELDS), 2 * len(engine.REPLICA_GROUP_FIELDS))
    assert engine.RSEL_BY == dict(err=0, lat=1, tail=2, share=3) and engine.RSEL_SIDE == {"in": 4, "out": 8}
    assert (engine.REPL_JUDGED_OUT, engine.REPL_ERR_OUT, engine.REPL_LAT_OUT, engine.REPL_TAIL_OUT) == tuple(
        x << 4 for x in (engine.REPL_JUDGED_IN, engine.REPL_ERR_IN, engine.REPL_LAT_IN, engine.REPL_TAIL_IN))


def test_set_replicas(g):
    cfn = "sg_set_replicas"
    assert g.set_replicas() == engine.REPLICA_DEFAULTS                # every default
    g.set_replicas(min_replicas=5, min_requests=1 << 40, tail_permille=990)
    g.set_replicas(dict(min_err_excess_q20=7), min_lat_ratio_q10=9, min_tail_bins=1)
    g.set_replicas({}, reserved=(0, 3))
    assert g._l.take() == [(cfn, "h", _packed()), (cfn, "h", _packed(min_replicas=5, min_requests=1 << 40, tail_permille=990)),
                           (cfn, "h", _packed(min_err_excess_q20=7, min_lat_ratio_q10=9, min_tail_bins=1)), (cfn, "h", _packed(reserved=(0, 3)))]
    assert g.set_replicas(None) is None                               # off
    assert g._l.take() == [(cfn, "h", None)]
    with pytest.raises(TypeError) as ei:
        g.set_replicas(None, min_replicas=3)
    assert str(ei.value) == "set_replicas(None) switches the replica outliers off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_replicas(dict(zzz=1), shift=2)
    assert str(ei.value) == "unknown replica parameters: ['shift', 'zzz']"
    assert g._l.take() == []
    text = b"sg_set_replicas: the workload rows are off (sg_set_group_nodes)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_replicas()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


READS = [("window_replicas", "sg_window_replicas", ROW), ("window_group_replicas", "sg_window_group_replicas", GROUP_ROW)]


@pytest.mark.parametrize("method,cfn,row", READS, ids=[r[0] for r in READS])
def test_indexed_reads(g, method, cfn, row):
    call = getattr(g, method)
    same(call(), row, pattern(row, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    a = call(index=None)
    same(a, row, pattern(row, 3))
    assert a.shape == (3, row.shape[0]) and a.dtype == np.dtype("<u4")
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    g._l.script[cfn] = dict(out=[2])
    same(call(index=[2, 0]), row, pattern(row, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    text = cfn.encode() + b": the last read window was closed while the replica outliers were off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value).endswith(text.decode())


def test_the_buffers(g):
    cfn = "sg_window_replicas_buffer"
    g._l.script = {cfn: dict(out=[0x3000, 0x4000])}
    assert g.window_replicas_buffer() == (0x3000, 0x4000)
    assert g._l.take() == [(cfn, "h", "out", "out")]


def test_the_selection(g):
    cfn, count, dtype = "sg_window_replicas_top", "sg_window_nodes", engine.NODE_DTYPE
    g._l.script = {cfn: dict(out=[5, 6]), count: dict(out=[4])}
    rows, idx, n = g.window_replicas_top(3, 1024)                     # cap = k; the default key: the error excess of the in side
    assert g._l.take() == [(cfn, "h", 0 | 4, 3, 1024, "buf", "buf", 3, "out", "out")]
    same(rows, dtype, pattern(dtype, 3)); same(idx, U4, pattern(U4, 3))
    assert rows.dtype == dtype and n == 6 and type(n) is int
    for by, b in engine.RSEL_BY.items():
        for side, sb in engine.RSEL_SIDE.items():
            g.window_replicas_top(2, by=by, side=side, cap=9)
            assert g._l.take() == [(cfn, "h", b | sb, 2, 0, "buf", "buf", 9, "out", "out")]
    g.window_replicas_top(2, by=9, cap=9)                             # the SG_RSEL_* int as it is
    assert g._l.take() == [(cfn, "h", 9, 2, 0, "buf", "buf", 9, "out", "out")]
    g.window_replicas_top(0)                                          # k = 0: the window's node count
    calls = g._l.take()
    assert calls[-1] == (cfn, "h", 4, 0, 0, "buf", "buf", 4, "out", "out") and len(calls) == 2
    with pytest.raises(ValueError):
        g.window_replicas_top(3, by="p99")
    with pytest.raises(ValueError):
        g.window_replicas_top(3, by="err", side="both")
    text = cfn.encode() + b": the replica outliers are off (sg_set_replicas)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_replicas_top(1)
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()
