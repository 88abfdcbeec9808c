"""The front end's methods of the workload tracks (K19) against the recording stand-in of tests/test_engine_front.py: the C calls
they make, what they return and the texts of their errors."""
import struct

import pytest

from alaz_amd import engine
from tests import engine_front as front

same, pattern = front.same, front.pattern
H, O, S, SO = front.H, front.O, front.S, front.SO
NEW_ABI = {
    "sg_set_group_tracks": [H, S], "sg_window_group_incident_tracks": front._COUNTED(engine.TRACK_DTYPE),
    "sg_window_group_tracks_ended": front._COUNTED(engine.TRACK_ENTRY_DTYPE), "sg_window_group_tracks_buffer": [H, O, O, O],
    "sg_group_track_entries": front._COUNTED(engine.TRACK_ENTRY_DTYPE), "sg_group_track_stats_get": [H, SO],
}
TWIN = {"sg_set_group_tracks": "sg_set_tracks", "sg_window_group_incident_tracks": "sg_window_incident_tracks",
        "sg_window_group_tracks_ended": "sg_window_tracks_ended", "sg_window_group_tracks_buffer": "sg_window_tracks_buffer",
        "sg_group_track_entries": "sg_track_entries", "sg_group_track_stats_get": "sg_track_stats_get"}


g = front.abi_fixture(NEW_ABI)


def _bytes(**over):
    return struct.pack("<4I", over.get("struct_size", 16), over.get("quiet_windows", 2), over.get("max_tracks", 0), over.get("reserved", 0))


def test_the_new_c_functions_are_in_the_signature_table():
    assert set(NEW_ABI) <= set(engine.EXPORTS) and len(NEW_ABI) == 6 and set(TWIN) == set(NEW_ABI)
    for name in NEW_ABI:
        assert len(engine._SIGNATURES[name][1]) == len(NEW_ABI[name]), name
        assert engine._SIGNATURES[name] == engine._SIGNATURES[TWIN[name]], name    # K13's shapes, call for call


def test_set_group_tracks(g):
    assert engine.TRACK_DEFAULTS == dict(quiet_windows=2, max_tracks=0)
    assert g.set_group_tracks() is None and g.set_group_tracks(dict(quiet_windows=0), max_tracks=12) is None
    assert g.set_group_tracks(None) is None and g.set_group_tracks(quiet_windows=5) is None
    assert g.set_group_tracks(quiet_windows=99, struct_size=8, reserved=7) is None   # a number goes to the library as it is
    cfn = "sg_set_group_tracks"
    assert g._l.take() == [(cfn, "h", _bytes()), (cfn, "h", _bytes(quiet_windows=0, max_tracks=12)), (cfn, "h", None),
                           (cfn, "h", _bytes(quiet_windows=5)), (cfn, "h", _bytes(quiet_windows=99, struct_size=8, reserved=7))]
    with pytest.raises(TypeError) as ei:
        g.set_group_tracks(None, quiet_windows=1)
    assert str(ei.value) == "set_group_tracks(None) switches workload tracking off and takes no parameters"
    with pytest.raises(TypeError) as ei:
        g.set_group_tracks(zzz=1)
    assert str(ei.value) == "unknown workload track parameters: ['zzz']"
    assert g._l.take() == []
    text = b"sg_set_group_tracks: the workload incidents are off (sg_set_group_incidents)"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_group_tracks()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: " + text.decode()


COUNTED = [("window_group_incident_tracks", "sg_window_group_incident_tracks", engine.TRACK_DTYPE),
           ("window_group_tracks_ended", "sg_window_group_tracks_ended", engine.TRACK_ENTRY_DTYPE),
           ("group_track_entries", "sg_group_track_entries", engine.TRACK_ENTRY_DTYPE)]


@pytest.mark.parametrize("method,cfn,dt", COUNTED, ids=[c[0] for c in COUNTED])
def test_counted_readbacks(g, method, cfn, dt):
    same(getattr(g, method)(), dt, pattern(dt, 0))
    assert g._l.take() == [(cfn, "h", None, 0, "out")]
    g._l.script[cfn] = dict(out=[3])
    same(getattr(g, method)(), dt, pattern(dt, 3))
    assert g._l.take() == [(cfn, "h", None, 0, "out"), (cfn, "h", "buf", 3, "out")]
    text = cfn.encode() + b": the last read window was closed while workload tracking was off"
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=text)}
    with pytest.raises(engine.ServiceGraphError) as ei:
        getattr(g, method)()
    assert str(ei.value) == "servicegraph rc=-71: " + text.decode()


def test_window_group_tracks_buffer(g):
    cfn = "sg_window_group_tracks_buffer"
    g._l.script = {cfn: dict(out=[0x1000, 0x2000, 0x3000])}
    assert g.window_group_tracks_buffer() == (0x1000, 0x2000, 0x3000)
    assert g._l.take() == [(cfn, "h", "out", "out", "out")]
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_group_tracks_buffer()
    assert str(ei.value) == "servicegraph rc=-71: off"


def test_group_track_stats(g):
    cfn = "sg_group_track_stats_get"
    g._l.script[cfn] = dict(fields=dict(windows=4, live=3, opened=9, dropped_cap=8))
    s = g.group_track_stats()
    assert g._l.take() == [(cfn, "h", "out:SgTrackStats")] and type(s) is engine.SgTrackStats
    assert (s.windows, s.live, s.opened, s.dropped_cap) == (4, 3, 9, 8)
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"sg_group_track_stats_get: workload tracking is off (sg_set_group_tracks)")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.group_track_stats()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value).endswith("workload tracking is off (sg_set_group_tracks)")


def test_k13s_methods_still_call_k13(g):
    g.set_tracks(); g.window_incident_tracks(); g.window_tracks_ended(); g.window_tracks_buffer(); g.track_entries(); g.track_stats()
    assert [c[0] for c in g._l.take()] == ["sg_set_tracks", "sg_window_incident_tracks", "sg_window_tracks_ended", "sg_window_tracks_buffer",
                                           "sg_track_entries", "sg_track_stats_get"]


def test_the_stage_shares_k13s_struct_and_defaults():
    st = engine._STAGES
    assert st["group_tracks"].struct is st["tracks"].struct is engine.SgTrackParams
    assert st["group_tracks"].defaults is st["tracks"].defaults is engine.TRACK_DEFAULTS
    assert st["group_tracks"].call == "sg_set_group_tracks" and st["group_tracks"].noun == "workload track"
    assert st["group_tracks"].off == "set_group_tracks(None) switches workload tracking off"
    assert engine.ABI_VERSION == 6
