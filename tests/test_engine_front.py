"""CPU tests of the ctypes front end (alaz_amd/engine.py) without the library: a ServiceGraph built by hand talks to a
recording stand-in for libservicegraph.so.  For every public method that only marshals — the set_* switches, the counted
and indexed readbacks, the capped flushes, the selections, the *_buffer and *_stats calls — the test pins the exact sequence
of C calls with their decoded arguments, what comes back (dtype, shape, contents the stand-in wrote) and, on the error paths,
the exception type and its whole text.

Decoded: the handle as "h", ints and floats as themselves, NULL as None, byref(struct) as the struct's bytes, a scalar
out-parameter as "out", a stats struct as "out:<class>", a buffer the library writes as "buf" once it is known to be non-null
and at least cap x itemsize bytes long (the stand-in sees every array the front end allocates), a buffer the library reads
as ("in", its values)."""
import ctypes as C
import struct

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE, EVENT_DTYPE
from tests.engine_front import HIST, INF, Lib, Numpy, U4, pattern, same


@pytest.fixture
def g(monkeypatch):
    spans = []
    monkeypatch.setattr(engine, "np", Numpy(spans))
    g = object.__new__(engine.ServiceGraph)
    g._h = C.c_void_p(0x5A5A)
    g.layers, g.max_edges, g.max_batch, g.rank, g.world = 2, 100, 1 << 16, 0, 1
    g._l = Lib(g._h, spans)
    yield g
    g._h = None                            # (nothing to destroy)


# ---- the set_* switches ---------------------------------------------------------------------------------------------------------
class Stage:
    def __init__(self, method, cfn, fmt, fields, off_text, noun, sample, reserved=True):
        self.method, self.cfn, self.fmt, self.fields, self.off_text, self.noun, self.sample = method, cfn, fmt, fields, off_text, noun, sample
        self.reserved = reserved

    def packed(self, **over):
        """the struct's bytes: struct_size, the fields in struct order (defaults unless overridden), reserved"""
        v = [over.get("struct_size", struct.calcsize(self.fmt))] + [over.get(f, d) for f, d in self.fields]
        if self.reserved:
            r = over.get("reserved", 0)
            v += list(r) if isinstance(r, tuple) else [r]
            v += [0] * (len(struct.unpack(self.fmt, bytes(struct.calcsize(self.fmt)))) - len(v))     # (sg_group_params: reserved[2])
        return struct.pack(self.fmt, *v)


_TREND = [("shift", 4), ("warmup", 4), ("ttl", 64), ("max_entries", 0), ("lat_floor_ns", 1000), ("err_floor", 10486)]
STAGES = [
    Stage("set_trend", "sg_set_trend", "<4I2Q2I", _TREND, "set_trend(None) switches the trend off", "trend", dict(shift=2, ttl=9)),
    Stage("set_node_trend", "sg_set_node_trend", "<4I2Q2I", _TREND, "set_node_trend(None) switches the node trend off", "node trend",
          dict(warmup=1, max_entries=1 << 33)),
    Stage("set_vanished", "sg_set_vanished", "<4I", [("silent_windows", 0), ("min_seen", 0), ("max_rows", 0)],
          "set_vanished(None) switches the list off", "vanished", dict(silent_windows=2, max_rows=7), reserved=False),
    Stage("set_rank", "sg_set_rank", "<4IfI", [("iters", 0), ("damping_q8", 0), ("seed", 0), ("seed_min_score", 0.0)],
          "set_rank(None) switches the ranking off", "rank", dict(iters=5, seed_min_score=0.25)),
    Stage("set_incidents", "sg_set_incidents", "<IIfI", [("by", 0), ("min_value", 0.0)],
          "set_incidents(None) switches the incidents off", "incident", dict(min_value=0.5)),
    Stage("set_tracks", "sg_set_tracks", "<4I", [("quiet_windows", 2), ("max_tracks", 0)],
          "set_tracks(None) switches tracking off", "track", dict(quiet_windows=0, max_tracks=12)),
    Stage("set_groups", "sg_set_groups", "<4I", [("max_groups", 0)], "set_groups(None) switches the groups off", "group",
          dict(max_groups=64)),
]
_STAGE_IDS = [s.method for s in STAGES]


def _armed(g, st):
    if st.method == "set_vanished":        # set_vanished reads what set_trend recorded
        g.set_trend()
        g._l.take()
    return getattr(g, st.method)


@pytest.mark.parametrize("st", STAGES, ids=_STAGE_IDS)
def test_set_stage_on_with_defaults_a_dict_keywords_or_both(g, st):
    call = _armed(g, st)
    assert call() is None
    assert g._l.take() == [(st.cfn, "h", st.packed())]
    assert call(dict(st.sample)) is None
    assert g._l.take() == [(st.cfn, "h", st.packed(**st.sample))]
    assert call(**st.sample) is None
    assert g._l.take() == [(st.cfn, "h", st.packed(**st.sample))]
    k0, v0 = list(st.sample.items())[0]
    other = {f: 3 for f, _ in st.fields[-1:] if f != k0}        # (another field, where the struct has one)
    both = {k0: v0, **other}
    assert call({k0: 99, **other}, **{k0: v0}) is None          # a keyword wins over the dict
    assert g._l.take() == [(st.cfn, "h", st.packed(**both))]
    assert call({}) is None and call(()) is None                # an empty dict or tuple: every default
    assert g._l.take() == [(st.cfn, "h", st.packed())] * 2


@pytest.mark.parametrize("st", STAGES, ids=_STAGE_IDS)
def test_set_stage_off_and_its_type_errors(g, st):
    call = _armed(g, st)
    assert call(None) is None
    assert g._l.take() == [(st.cfn, "h", None)]
    with pytest.raises(TypeError) as ei:
        call(None, **st.sample)
    assert str(ei.value) == f"{st.off_text} and takes no parameters"
    with pytest.raises(TypeError) as ei:
        call(dict(zzz=1), aaa=2, **st.sample)
    assert str(ei.value) == f"unknown {st.noun} parameters: ['aaa', 'zzz']"
    assert g._l.take() == []                                    # neither reached the library


@pytest.mark.parametrize("st", STAGES, ids=_STAGE_IDS)
def test_set_stage_takes_the_callers_struct_size_and_reserved(g, st):
    call = _armed(g, st)
    call(struct_size=8)
    assert g._l.take() == [(st.cfn, "h", st.packed(struct_size=8))]
    if st.reserved:
        call(dict(reserved=7), struct_size=12)
        assert g._l.take() == [(st.cfn, "h", st.packed(struct_size=12, reserved=7))]


def test_set_vanished_has_no_reserved_field(g):
    g.set_trend()
    g._l.take()
    with pytest.raises(TypeError) as ei:
        g.set_vanished(reserved=0)
    assert str(ei.value) == "unknown vanished parameters: ['reserved']"
    assert g._l.take() == []


def test_set_stage_raises_what_the_library_refuses(g):
    g._l.script = {"sg_set_tracks": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"incidents are off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.set_tracks()
    assert ei.value.rc == engine.SG_ESTATE and str(ei.value) == "servicegraph rc=-71: incidents are off"
    with pytest.raises(engine.ServiceGraphError):
        g.set_tracks(None)


def test_set_rank_seed_by_name_or_number(g):
    rank = STAGES[3]
    g.set_rank(seed="uniform")
    g.set_rank(seed=1)
    g.set_rank(dict(seed="score"), iters=3)
    assert g._l.take() == [("sg_set_rank", "h", rank.packed(seed=1))] * 2 + [("sg_set_rank", "h", rank.packed(iters=3))]
    with pytest.raises(ValueError) as ei:
        g.set_rank(seed="x")
    assert str(ei.value) == "seed must be one of ['score', 'uniform'], not 'x'"
    with pytest.raises(TypeError) as ei:                        # the unknown key is reported before the bad seed
        g.set_rank(seed="x", bogus=1)
    assert str(ei.value) == "unknown rank parameters: ['bogus']"
    assert g._l.take() == []


def test_set_incidents_key_by_name_or_number(g):
    inc = STAGES[4]
    g.set_incidents(by="lat_dev")
    g.set_incidents(by=2)
    g.set_incidents(dict(by="new", min_value=1.5))
    g.set_incidents(by=9)                                       # a number goes to the library as it is
    assert g._l.take() == [("sg_set_incidents", "h", inc.packed(by=1)), ("sg_set_incidents", "h", inc.packed(by=2)),
                           ("sg_set_incidents", "h", inc.packed(by=3, min_value=1.5)), ("sg_set_incidents", "h", inc.packed(by=9))]
    with pytest.raises(ValueError) as ei:
        g.set_incidents(by="x")
    assert str(ei.value) == "by must be one of ['err_dev', 'lat_dev', 'new', 'score'], not 'x'"
    assert g._l.take() == []


def test_set_groups_reserved_as_an_int_or_a_pair(g):
    grp = STAGES[6]
    g.set_groups(reserved=5)
    g.set_groups(reserved=(1, 2))
    g.set_groups(reserved=[3, 4])
    assert g._l.take() == [("sg_set_groups", "h", struct.pack("<4I", 16, 0, 5, 0)), ("sg_set_groups", "h", struct.pack("<4I", 16, 0, 1, 2)),
                           ("sg_set_groups", "h", struct.pack("<4I", 16, 0, 3, 4))]
    assert grp.packed() == struct.pack("<4I", 16, 0, 0, 0)


def test_struct_sizes_the_switches_send():
    assert [struct.calcsize(s.fmt) for s in STAGES] == [40, 40, 16, 24, 16, 16, 16]


# ---- the vanished list's clip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_edges,rows", [(100, 200), (40000, 65536), (0, 2)])
def test_window_vanished_clips_to_what_set_trend_and_set_vanished_recorded(g, max_edges, rows):
    """set_trend(max_entries=0) records min(2^31, 2 x max(max_edges, 1)) entries, set_vanished() min(65536, that) rows"""
    g.max_edges = max_edges
    g.set_trend(max_entries=0)
    g.set_vanished()
    g._l.take()
    g._l.script["sg_window_vanished"] = dict(out=[rows + 3])
    got = g.window_vanished()
    assert g._l.take() == [("sg_window_vanished", "h", None, 0, "out"), ("sg_window_vanished", "h", "buf", rows + 3, "out")]
    same(got, engine.VANISHED_DTYPE, pattern(engine.VANISHED_DTYPE, rows))


def test_window_vanished_clip_follows_max_entries_and_max_rows(g):
    g.set_trend(max_entries=4)
    g.set_vanished()
    g._l.script["sg_window_vanished"] = dict(out=[9])
    assert len(g.window_vanished()) == 4
    g.set_vanished(max_rows=3)
    g._l.script["sg_window_vanished"] = dict(out=[5])
    g._l.take()
    rows, n = g.window_vanished(with_count=True)
    assert g._l.take() == [("sg_window_vanished", "h", None, 0, "out"), ("sg_window_vanished", "h", "buf", 5, "out")]
    same(rows, engine.VANISHED_DTYPE, pattern(engine.VANISHED_DTYPE, 3))
    assert n == 5 and type(n) is int
    g._l.script["sg_window_vanished"] = dict(out=[0])
    rows, n = g.window_vanished(with_count=True)
    assert g._l.take() == [("sg_window_vanished", "h", None, 0, "out")]
    same(rows, engine.VANISHED_DTYPE, pattern(engine.VANISHED_DTYPE, 0))
    assert n == 0


def test_set_vanished_before_any_set_trend_fails_after_the_call(g):
    """(what the front end does today: the library refuses the call first — SG_ESTATE, the trend is off — so this is only
    reached against a stand-in)"""
    with pytest.raises(AttributeError):
        g.set_vanished()
    assert g._l.take() == [("sg_set_vanished", "h", STAGES[2].packed())]


# ---- counted readbacks: the count, then the rows --------------------------------------------------------------------------------
COUNTED = [
    ("window_nodes", "sg_window_nodes", engine.NODE_DTYPE), ("window_incidents", "sg_window_incidents", engine.INCIDENT_DTYPE),
    ("trend_entries", "sg_trend_entries", engine.TREND_ENTRY_DTYPE), ("node_trend_entries", "sg_node_trend_entries", engine.TREND_ENTRY_DTYPE),
    ("outbound_ips", "sg_window_outbound_ips", U4), ("window_hist", "sg_window_hist", HIST),
    ("window_incident_tracks", "sg_window_incident_tracks", engine.TRACK_DTYPE),
    ("window_tracks_ended", "sg_window_tracks_ended", engine.TRACK_ENTRY_DTYPE), ("track_entries", "sg_track_entries", engine.TRACK_ENTRY_DTYPE),
    ("window_groups", "sg_window_groups", engine.GROUP_EDGE_DTYPE), ("window_group_perm", "sg_window_group_perm", U4),
]


@pytest.mark.parametrize("method,cfn,dtype", COUNTED, ids=[c[0] for c in COUNTED])
def test_counted_readback(g, method, cfn, dtype):
    got = getattr(g, method)()                                  # n = 0: one call, an empty result of the right dtype and shape
    assert g._l.take() == [(cfn, "h", None, 0, "out")]
    same(got, dtype, pattern(dtype, 0))
    g._l.script[cfn] = dict(out=[3])
    got = getattr(g, method)()
    assert g._l.take() == [(cfn, "h", None, 0, "out"), (cfn, "h", "buf", 3, "out")]
    same(got, dtype, pattern(dtype, 3))
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"stage off")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        getattr(g, method)()
    assert str(ei.value) == "servicegraph rc=-71: stage off" and ei.value.rc == -71
    assert g._l.take() == [(cfn, "h", None, 0, "out"), ("sg_last_error", "h")]


def test_window_hist_has_sixteen_bins_per_row(g):
    g._l.script["sg_window_hist"] = dict(out=[3])
    h = g.window_hist()
    assert h.shape == (3, 16) and h.dtype == np.uint32 and h[2].tolist() == [0x03030303] * 16
    g._l.script = {}
    assert g.outbound_ips().shape == (0,) and g.window_hist().shape == (0, 16)


# ---- indexed readbacks: every row, or the rows at index -------------------------------------------------------------------------
INDEXED = [
    ("window_trend", "sg_window_trend", engine.TREND_DTYPE), ("window_node_trend", "sg_window_node_trend", engine.NODE_TREND_DTYPE),
    ("window_rank", "sg_window_rank", engine.RANK_DTYPE), ("window_node_incident", "sg_window_node_incident", U4),
    ("window_row_group", "sg_window_row_group", U4),
]


@pytest.mark.parametrize("method,cfn,dtype", INDEXED, ids=[c[0] for c in INDEXED])
def test_indexed_readback(g, method, cfn, dtype):
    call = getattr(g, method)
    got = call()                                                # index=None, n = 0
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out")]
    same(got, dtype, pattern(dtype, 0))
    g._l.script[cfn] = dict(out=[3])
    got = call(index=None)
    assert g._l.take() == [(cfn, "h", None, 0, None, 0, "out"), (cfn, "h", None, 0, "buf", 3, "out")]
    same(got, dtype, pattern(dtype, 3))
    got = call(index=[])                                        # no C call at all
    assert g._l.take() == []
    same(got, dtype, pattern(dtype, 0))
    g._l.script[cfn] = dict(out=[2])
    got = call(index=[2, 0])
    assert g._l.take() == [(cfn, "h", ("in", [2, 0]), 2, "buf", 2, "out")]
    same(got, dtype, pattern(dtype, 2))
    got = call(np.array([1], dtype=np.int64))                   # any integer array: converted to u32
    assert g._l.take() == [(cfn, "h", ("in", [1]), 1, "buf", 1, "out")]
    assert len(got) == 1


# ---- capped flushes -------------------------------------------------------------------------------------------------------------
CAPPED = [("flush_window", "sg_flush_window", (7,), (7,)), ("flush_end", "sg_flush_end", (), ()), ("window_read", "sg_window_read", (), ())]


@pytest.mark.parametrize("method,cfn,args,cargs", CAPPED, ids=[c[0] for c in CAPPED])
def test_capped_flush(g, method, cfn, args, cargs):
    g._l.script[cfn] = dict(out=[5])
    got = getattr(g, method)(*args)                             # cap=None: max_edges rows of room
    assert g._l.take() == [(cfn, "h", *cargs, "buf", 100, "out")]
    same(got, EDGE_OUT_DTYPE, pattern(EDGE_OUT_DTYPE, 5))
    got = getattr(g, method)(*args, cap=2)                      # the window has 5 rows: 2 come back
    assert g._l.take() == [(cfn, "h", *cargs, "buf", 2, "out")]
    same(got, EDGE_OUT_DTYPE, pattern(EDGE_OUT_DTYPE, 2))
    g._l.script[cfn] = dict(out=[0])
    same(getattr(g, method)(*args), EDGE_OUT_DTYPE, pattern(EDGE_OUT_DTYPE, 0))


def test_flush_window_defaults_to_window_end_zero(g):
    g.flush_window()
    assert g._l.take() == [("sg_flush_window", "h", 0, "buf", 100, "out")]


# ---- selections -----------------------------------------------------------------------------------------------------------------
TOPS = [("flush_window_top", "sg_flush_window_top", dict(window_end_ms=7), (7,)), ("flush_end_top", "sg_flush_end_top", {}, ())]


@pytest.mark.parametrize("method,cfn,kw,lead", TOPS, ids=[c[0] for c in TOPS])
def test_edge_selection_flush(g, method, cfn, kw, lead):
    call = getattr(g, method)
    g._l.script = {cfn: dict(out=[2, 9]), cfn + "_by": dict(out=[5, 11])}
    rows, idx, n = call(3, 0.5, by="score", **kw)               # the plain function, cap = k
    assert g._l.take() == [(cfn, "h", *lead, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, EDGE_OUT_DTYPE, pattern(EDGE_OUT_DTYPE, 2))
    same(idx, U4, pattern(U4, 2))
    assert n == 9 and type(n) is int
    rows, idx, n = call(3, 0.5, by="err_dev", **kw)             # the _by function with SG_SEL_ERR_DEV; 5 selected, 3 fit
    assert g._l.take() == [(cfn + "_by", "h", *lead, 2, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, EDGE_OUT_DTYPE, pattern(EDGE_OUT_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 11
    rows, idx, n = call(0, **kw)                                # k = 0, cap=None: max_edges; min_score defaults to -inf
    assert g._l.take() == [(cfn, "h", *lead, 0, INF, "buf", "buf", 100, "out", "out")]
    assert len(rows) == len(idx) == 2
    rows, idx, n = call(8, cap=1, by="new", **kw)
    assert g._l.take() == [(cfn + "_by", "h", *lead, 3, 8, INF, "buf", "buf", 1, "out", "out")]
    assert len(rows) == len(idx) == 1 and n == 11
    for bad in ("x", 2):                                        # a key is a name here, never a number
        with pytest.raises(ValueError) as ei:
            call(3, by=bad, **kw)
        assert str(ei.value) == f"by must be one of ['err_dev', 'lat_dev', 'new', 'score'], not {bad!r}"
    assert g._l.take() == []


def test_flush_window_top_defaults_to_window_end_zero(g):
    g.flush_window_top(4)
    assert g._l.take() == [("sg_flush_window_top", "h", 0, 4, INF, "buf", "buf", 4, "out", "out")]


def test_window_select(g):
    assert g.window_select(3, 0.5, 0x1000, 0x2000, 8, 0x3000, stream=0x4000, by="score") is None
    assert g.window_select(3, 0.5, 0x1000, 0, 8, 0x3000) is None                    # no index wanted, the window's stream
    assert g.window_select(0, 1.5, 0x1000, 0x2000, 8, 0x3000, by="err_dev") is None
    assert g._l.take() == [("sg_window_select", "h", 3, 0.5, 0x1000, 0x2000, 8, 0x3000, 0x4000),
                           ("sg_window_select", "h", 3, 0.5, 0x1000, None, 8, 0x3000, None),
                           ("sg_window_select_by", "h", 2, 0, 1.5, 0x1000, 0x2000, 8, 0x3000, None)]
    with pytest.raises(ValueError) as ei:
        g.window_select(3, 0.5, 0x1000, 0, 8, 0x3000, by="x")
    assert str(ei.value) == "by must be one of ['err_dev', 'lat_dev', 'new', 'score'], not 'x'"


def test_window_nodes_top(g):
    g._l.script = {"sg_window_nodes_top": dict(out=[5, 6]), "sg_window_nodes": dict(out=[4])}
    rows, idx, n = g.window_nodes_top(3, 0.5, by="in_err_dev")                      # cap = k
    assert g._l.take() == [("sg_window_nodes_top", "h", 2, 3, 0.5, "buf", "buf", 3, "out", "out")]
    same(rows, engine.NODE_DTYPE, pattern(engine.NODE_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 6 and type(n) is int
    rows, idx, n = g.window_nodes_top(0)                                            # k = 0, cap=None: the window's node count
    assert g._l.take() == [("sg_window_nodes", "h", None, 0, "out"), ("sg_window_nodes_top", "h", 0, 0, INF, "buf", "buf", 4, "out", "out")]
    assert len(rows) == len(idx) == 4 and n == 6
    rows, idx, n = g.window_nodes_top(0, cap=9, by="new")
    assert g._l.take() == [("sg_window_nodes_top", "h", 5, 0, INF, "buf", "buf", 9, "out", "out")]
    assert len(rows) == len(idx) == 5
    g._l.script["sg_window_nodes"] = dict(out=[0])                                  # a window without nodes
    rows, idx, n = g.window_nodes_top(0)
    assert g._l.take()[1] == ("sg_window_nodes_top", "h", 0, 0, INF, "buf", "buf", 0, "out", "out")
    assert len(rows) == len(idx) == 0 and rows.dtype == engine.NODE_DTYPE
    with pytest.raises(ValueError) as ei:
        g.window_nodes_top(3, by="lat_dev")
    assert str(ei.value) == "by must be one of ['in_err_dev', 'in_lat_dev', 'new', 'out_err_dev', 'out_lat_dev', 'score'], not 'lat_dev'"
    assert g._l.take() == []


def test_window_rank_top(g):
    g._l.script = {"sg_window_rank_top": dict(out=[5, 6]), "sg_window_nodes": dict(out=[4])}
    rows, rk, idx, n = g.window_rank_top(3, 0.25)
    assert g._l.take() == [("sg_window_rank_top", "h", 3, 0.25, "buf", "buf", "buf", 3, "out", "out")]
    same(rows, engine.NODE_DTYPE, pattern(engine.NODE_DTYPE, 3))
    same(rk, engine.RANK_DTYPE, pattern(engine.RANK_DTYPE, 3))
    same(idx, U4, pattern(U4, 3))
    assert n == 6 and type(n) is int
    rows, rk, idx, n = g.window_rank_top(0)
    assert g._l.take() == [("sg_window_nodes", "h", None, 0, "out"),
                           ("sg_window_rank_top", "h", 0, INF, "buf", "buf", "buf", 4, "out", "out")]
    assert len(rows) == len(rk) == len(idx) == 4
    rows, rk, idx, n = g.window_rank_top(2, cap=9)
    assert g._l.take() == [("sg_window_rank_top", "h", 2, INF, "buf", "buf", "buf", 9, "out", "out")]
    assert len(rows) == len(rk) == len(idx) == 5


def test_device_resident_node_selections(g):
    g.window_nodes_select(3, 0.5, 0x1000, 0, 8, 0x3000, by="out_lat_dev")
    g.window_rank_select(3, 0.5, 0, 0x2000, 8, 0x3000, stream=0x4000)
    assert g._l.take() == [("sg_window_nodes_select", "h", 3, 3, 0.5, 0x1000, None, 8, 0x3000, None),
                           ("sg_window_rank_select", "h", 3, 0.5, None, 0x2000, 8, 0x3000, 0x4000)]


# ---- device pointers and statistics ---------------------------------------------------------------------------------------------
BUFFERS = [("trend_buffer", "sg_window_trend_buffer", 1), ("node_trend_buffer", "sg_window_node_trend_buffer", 1),
           ("rank_buffer", "sg_window_rank_buffer", 1), ("rows_buffer", "sg_window_rows_buffer", 1),
           ("vanished_buffer", "sg_window_vanished_buffer", 2), ("nodes_buffer", "sg_window_nodes_buffer", 2),
           ("window_incidents_buffer", "sg_window_incidents_buffer", 3), ("window_tracks_buffer", "sg_window_tracks_buffer", 3),
           ("window_groups_buffer", "sg_window_groups_buffer", 4)]


@pytest.mark.parametrize("method,cfn,n", BUFFERS, ids=[b[0] for b in BUFFERS])
def test_buffer_pointers(g, method, cfn, n):
    ptrs = [0x10000 * (j + 1) for j in range(n)]
    g._l.script[cfn] = dict(out=ptrs)
    got = getattr(g, method)()
    assert g._l.take() == [(cfn, "h") + ("out",) * n]
    if n == 1:
        assert got == ptrs[0] and type(got) is int              # a plain int, no tuple
    else:
        assert got == tuple(ptrs) and type(got) is tuple and all(type(p) is int for p in got)
    g._l.script = {cfn: dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"no window")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        getattr(g, method)()
    assert str(ei.value) == "servicegraph rc=-71: no window"


def test_window_buffers_and_feat_buffer(g):
    g._l.script = {"sg_window_buffers": dict(out=[0x1000, 0x2000, 0x3000, 77]), "sg_window_feat_buffer": dict(out=[0x4000, 64])}
    assert g.window_buffers() == (0x1000, 0x2000, 0x3000, 77)
    assert g.feat_buffer(1) == (0x4000, 64)
    assert g._l.take() == [("sg_window_buffers", "h", "out", "out", "out", "out"), ("sg_window_feat_buffer", "h", 1, "out", "out")]


STATS = [("stats", "sg_stats_get", "SgStats", dict(events_in=5, last_window_tmin_ms=-3, last_window_new_edges=9)),
         ("trend_stats", "sg_trend_stats_get", "SgTrendStats", dict(windows=2, dropped=4)),
         ("node_trend_stats", "sg_node_trend_stats_get", "SgTrendStats", dict(entries=7, expired=1)),
         ("track_stats", "sg_track_stats_get", "SgTrackStats", dict(live=3, dropped_cap=8))]


@pytest.mark.parametrize("method,cfn,cls,fields", STATS, ids=[s[0] for s in STATS])
def test_stats(g, method, cfn, cls, fields):
    g._l.script[cfn] = dict(fields=fields)
    s = getattr(g, method)()
    assert g._l.take() == [(cfn, "h", "out:" + cls)]
    assert type(s) is getattr(engine, cls)
    assert {n: getattr(s, n) for n, _ in s._fields_} == {**{n: 0 for n, _ in s._fields_}, **fields}
    g._l.script = {cfn: dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=b"bad handle")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        getattr(g, method)()
    assert str(ei.value) == "servicegraph rc=-22: bad handle" and ei.value.rc == engine.SG_EINVAL


# ---- return codes ---------------------------------------------------------------------------------------------------------------
def test_a_nonzero_return_code_raises_with_rc_and_the_librarys_text(g):
    g._l.script = {"sg_window_nodes": dict(rc=engine.SG_ESTATE), "sg_last_error": dict(text=b"wrong phase")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.window_nodes()
    assert isinstance(ei.value, RuntimeError) and ei.value.rc == -71 and str(ei.value) == "servicegraph rc=-71: wrong phase"
    assert g._l.take() == [("sg_window_nodes", "h", None, 0, "out"), ("sg_last_error", "h")]
    g._l.script = {"sg_flush_window": dict(rc=engine.SG_ENOSPC), "sg_last_error": dict(text=None)}      # a NULL string reads as an empty one
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.flush_window()
    assert str(ei.value) == "servicegraph rc=-28: " and ei.value.rc == engine.SG_ENOSPC


def test_ingest_hands_a_full_ring_back_instead_of_raising(g):
    ev = np.zeros(2, dtype=EVENT_DTYPE)
    ev["saddr"], ev["duration_ns"] = [1, 2], [1000, 1 << 40]
    assert g.ingest(ev) == 0
    g._l.script["sg_ingest"] = dict(rc=engine.SG_EAGAIN)
    assert g.ingest(ev) == engine.SG_EAGAIN == -11
    assert g._l.take() == [("sg_ingest", "h", ("in", ev.tolist()), 2)] * 2          # no sg_last_error: nothing was raised
    g._l.script = {"sg_ingest": dict(rc=engine.SG_EINVAL), "sg_last_error": dict(text=b"n > max_batch")}
    with pytest.raises(engine.ServiceGraphError) as ei:
        g.ingest(ev)
    assert str(ei.value) == "servicegraph rc=-22: n > max_batch"
