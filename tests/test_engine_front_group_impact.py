"""The front end's methods of the workload impact (K22) against the recording stand-in of tests/test_engine_front.py: the C calls
they make, the shapes they return and the texts of their errors."""

import numpy as np
import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern = front.same, front.pattern
H, I, O = front.H, front.I, front.O
U4, U8 = np.dtype("<u4"), np.dtype("<u8")
ROW = np.dtype((U8, engine.IMPACT_WORDS))                             # one impact row
MASK2 = np.dtype((U8, 2))                                             # one mask row at W = 2
NEW_ABI = {
    "sg_set_group_impact": [H, I, I], "sg_window_group_impact": front._COUNTED(ROW), "sg_window_group_node_hops": front._INDEXED(U4),
    "sg_window_group_impact_mask": [H, front.Out(MASK2, 2), I, O, O], "sg_window_group_impact_buffer": [H, O, O, O, O],
}


g = front.abi_fixture(NEW_ABI)


def _raises(g, cfn, call, text):
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        call()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()
    g._l.take()


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 5
    for name in NEW_ABI:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
    assert engine._SIGNATURES["sg_window_group_node_hops"] == engine._SIGNATURES["sg_window_group_node_incident"]
    assert engine._SIGNATURES["sg_window_group_impact"] == engine._SIGNATURES["sg_window_group_incidents"]
    assert engine.ABI_VERSION == 6                                    # no new struct, no ABI bump
    assert not any(n.startswith("SgImpact") or (n.endswith("_DTYPE") and "IMPACT" in n) for n in dir(engine))


def test_the_constants_have_plain_names():
    assert (engine.IMPACT_WORDS, engine.IMPACT_MAX_INCIDENTS, engine.IMPACT_MAX_HOPS, engine.NO_HOPS) == (8, 1024, 64, 0xFFFFFFFF)
    assert engine.IMPACT_FIELDS == ("exposed", "direct", "far", "entries", "entry_count", "entry_err", "into_count", "into_err")
    assert [getattr(engine, "IMPACT_" + f.upper()) for f in engine.IMPACT_FIELDS] == list(range(8))


def test_set_group_impact(g):
    cfn = "sg_set_group_impact"
    assert g.set_group_impact() is None and g.set_group_impact(64) is None and g.set_group_impact(max_hops=3) is None
    assert g.set_group_impact(1024, 64) is None and g.set_group_impact(None) is None
    assert g.set_group_impact(0, 9) is None                          # a number goes to the library as it is
    assert g._l.take() == [(cfn, "h", 256, 8), (cfn, "h", 64, 8), (cfn, "h", 256, 3), (cfn, "h", 1024, 64), (cfn, "h", 0, 0), (cfn, "h", 0, 9)]
    _raises(g, cfn, g.set_group_impact, b"sg_set_group_impact: the workload incidents are off (sg_set_group_incidents)")
    g._l.script = {cfn: dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=b"sg_set_group_impact: bad parameters")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_impact(2000)
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith("sg_set_group_impact: bad parameters")


def test_window_group_impact(g):
    cfn = "sg_window_group_impact"
    got = g.window_group_impact()
    assert g._l.take() == [(cfn, "h", None, 0, "out")] and got.shape == (0, 8) and got.dtype == U8
    g._l.script[cfn] = dict(out=[3])
    got = g.window_group_impact()
    assert g._l.take() == [(cfn, "h", None, 0, "out"), (cfn, "h", "buf", 3, "out")]
    same(got, ROW, pattern(ROW, 3))
    assert got.shape == (3, 8)
    _raises(g, cfn, g.window_group_impact, b"sg_window_group_impact: the last read window was closed while the workload impact was off")


def test_window_group_node_hops(g):
    cfn = "sg_window_group_node_hops"
    got = g.window_group_node_hops()
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    same(got, U4, pattern(U4, 0))
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_node_hops(index=None), U4, pattern(U4, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(g.window_group_node_hops(index=[]), U4, pattern(U4, 0))
    assert g._l.take() == []                                          # no C call at all
    g._l.script[cfn] = dict(out=[2])
    same(g.window_group_node_hops([2, 0]), U4, pattern(U4, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    g._l.script = {cfn: dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=b"sg_window_group_node_hops: a node index beyond the window's workload rows")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_node_hops([99])
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith("a node index beyond the window's workload rows")


def test_window_group_impact_mask(g):
    cfn = "sg_window_group_impact_mask"
    g._l.script[cfn] = dict(out=[0, 2])
    got = g.window_group_impact_mask()
    assert g._l.take() == [(cfn, "h", None, 0, "out", "out")] and got.shape == (0, 2) and got.dtype == U8
    g._l.script[cfn] = dict(out=[5, 2])
    got = g.window_group_impact_mask()
    assert g._l.take() == [(cfn, "h", None, 0, "out", "out"), (cfn, "h", "buf", 5, "out", "out")]
    same(got, MASK2, pattern(MASK2, 5))
    assert got.shape == (5, 2)
    _raises(g, cfn, g.window_group_impact_mask, b"sg_window_group_impact_mask: the workload impact is off (sg_set_group_impact)")


def test_window_group_impact_buffer(g):
    cfn = "sg_window_group_impact_buffer"
    g._l.script = {cfn: dict(out=[0x1000, 0x2000, 0x3000, 0x4000])}
    assert g.window_group_impact_buffer() == (0x1000, 0x2000, 0x3000, 0x4000)
    assert g._l.take() == [(cfn, "h", "out", "out", "out", "out")]
    _raises(g, cfn, g.window_group_impact_buffer, b"sg_window_group_impact_buffer: the window was closed while the workload impact was off")
