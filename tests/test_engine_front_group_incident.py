"""The front end's methods of the workload incidents (K18) against the recording stand-in of tests/test_engine_front.py: the C calls
they make, what they return and the texts of their errors."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from tests.abi_layouts import LAYOUTS
from tests import engine_front as front

U4, same, pattern = front.U4, front.same, front.pattern
H, O, S = front.H, front.O, front.S
NEW_ABI = {
    "sg_set_group_incidents": [H, S], "sg_window_group_incidents": front._COUNTED(engine.INCIDENT_DTYPE),
    "sg_window_group_node_incident": front._INDEXED(U4), "sg_window_group_incidents_buffer": [H, O, O, O],
}


g = front.abi_fixture(NEW_ABI)


def _bytes(**over):
    return struct.pack("<IIfI", over.get("struct_size", 16), over.get("by", 0), over.get("min_value", 0.0), over.get("reserved", 0))


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 4
    twin = {"sg_set_group_incidents": "sg_set_incidents", "sg_window_group_incidents": "sg_window_incidents",
            "sg_window_group_node_incident": "sg_window_node_incident", "sg_window_group_incidents_buffer": "sg_window_incidents_buffer"}
    for name in NEW_ABI:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
        assert engine._SIGNATURES[name] == engine._SIGNATURES[twin[name]], name    # K12's shapes, call for call


def test_set_group_incidents(g):
    assert engine.INCIDENT_DEFAULTS == dict(by="score", min_value=0.0)
    assert g.set_group_incidents() is None and g.set_group_incidents(dict(by="lat_dev"), min_value=1.5) is None
    assert g.set_group_incidents(None) is None and g.set_group_incidents(by=2) is None
    assert g.set_group_incidents(by=9, struct_size=8, reserved=7) is None  # a number goes to the library as it is
    cfn = "sg_set_group_incidents"
    assert g._l.take() == [(cfn, "h", _bytes()), (cfn, "h", _bytes(by=1, min_value=1.5)), (cfn, "h", None), (cfn, "h", _bytes(by=2)),
                           (cfn, "h", _bytes(by=9, struct_size=8, reserved=7))]
    with pytest.raises(TypeError) as ei:
        g.set_group_incidents(None, by=1)
    assert str(ei.value) == "set_group_incidents(None) switches the workload incidents off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_incidents(zzz=1)
    assert str(ei.value) == "unknown workload incident parameters: ['zzz']"
    with pytest.raises(ValueError) as ei:
        g.set_group_incidents(by="x")
    assert str(ei.value) == "by must be one of ['err_dev', 'lat_dev', 'new', 'score'], not 'x'"
    assert g._l.take() == []
    text = b"sg_set_group_incidents by a trend key: the group trend is off (sg_set_group_trend)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_incidents(by="err_dev")
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_incidents_is_a_counted_readback(g):
    cfn, dt = "sg_window_group_incidents", engine.INCIDENT_DTYPE
    same(g.window_group_incidents(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_incidents(), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, "out"), (cfn, "h", "buf", 3, "out")]
    text = b"sg_window_group_incidents: the last read window was closed while the workload incidents were off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_incidents()
    assert str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_node_incident_is_an_indexed_readback(g):
    cfn = "sg_window_group_node_incident"
    same(g.window_group_node_incident(), U4, pattern(U4, 0))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(g.window_group_node_incident(index=None), U4, pattern(U4, 3))
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(g.window_group_node_incident(index=[]), U4, pattern(U4, 0))
    assert g._l.take() == []
    g._l.script[cfn] = dict(out=[2])
    same(g.window_group_node_incident([2, 0]), U4, pattern(U4, 2))
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    text = b"sg_window_group_node_incident: a node index beyond the window's workload rows"
    g._l.script = {cfn: dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_node_incident([7])
    assert ei.value.rc == engine.SG_EINVAL and str(ei.value).endswith(text.decode())


def test_window_group_incidents_buffer(g):
    cfn = "sg_window_group_incidents_buffer"
    g._l.script = {cfn: dict(out=[0x1000, 0x2000, 0x3000])}
    assert g.window_group_incidents_buffer() == (0x1000, 0x2000, 0x3000)
    assert g._l.take() == [(cfn, "h", "out", "out", "out")]
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_incidents_buffer()
    assert str(ei.value) == "servicegraph rc=-71: off"


def test_k12s_methods_still_call_k12(g):
    g.set_incidents(); g.window_incidents(); g.window_node_incident()
    assert [c[0] for c in g._l.take()] == ["sg_set_incidents", "sg_window_incidents", "sg_window_node_incident"]


def test_the_stage_adds_no_struct_and_no_constant():
    twins = {n: v for n, v in vars(engine).items() if (n.startswith("Sg") and isinstance(v, type) and issubclass(v, C.Structure))
             or (n.endswith("_DTYPE") and isinstance(v, np.dtype))}
    assert all(any(v is t for t in LAYOUTS.values()) for v in twins.values()) and len(twins) == len(LAYOUTS) == 23
    assert engine.ABI_VERSION == 6 and engine.NO_INCIDENT == 0xFFFFFFFF
    st = engine._STAGES
    assert st["group_incidents"].struct is st["incidents"].struct is engine.SgIncidentParams
    assert st["group_incidents"].defaults is st["incidents"].defaults is engine.INCIDENT_DEFAULTS
