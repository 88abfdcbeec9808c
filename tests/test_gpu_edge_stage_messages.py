"""The engine's own sg_last_error texts of the edge baselines, their vanished lists and the index selections, over the service-map
edges (K8, K7 by a trend key, the node selection) and over the group edges (K15, the group selection, the workload selection): the
return code and the exact text of every refusal these entry points have, as tests/test_gpu_stage_messages.py holds them for the
ranking and the incidents.  EXPECT is a literal table: the calls go to the C functions directly, so that no Python-side check or
helper call answers in the engine's place.  A text of None: the call sets none (sg_last_error still holds the previous one)."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine, replay
from alaz_amd.engine import SG_EINVAL, SG_ESTATE, SG_OK
from tests.gpu_scaffold import _engine, _feed

pytestmark = pytest.mark.gpu

#: call -> state -> (return code, sg_last_error).  States: below_off (the stage below off: the groups, the edge baseline or the
#: rollup), bad (bad parameters), bad_flush (bad parameters while a flush is open: which refusal comes first), unknown_key (by one
#: past the last, with everything off), kmax (k = SG_SELECT_MAX_K + 1), trend_key (a trend key with the baseline it reads off), off
#: (the stage off), was_below (a window closed while the stage below was off), was (a window closed while the stage was off; the
#: edge trend's two reads check neither and answer), beyond (an index equal to the window's row count), flush (between
#: sg_flush_begin and sg_flush_end; the calls that do not look at it answer)
EXPECT = {
    "edge": {
        "sg_set_trend": {
            "bad": (SG_EINVAL, "sg_set_trend: bad parameters"),
            "bad_flush": (SG_EINVAL, "sg_set_trend: bad parameters"),
            "flush": (SG_ESTATE, "sg_set_trend while a flush is open"),
        },
        "sg_window_trend": {
            "off": (SG_ESTATE, "sg_window_trend: the trend is off (sg_set_trend)"),
            "was": (SG_OK, None),
            "beyond": (SG_EINVAL, "sg_window_trend: a row index beyond the window's edges"),
            "flush": (SG_OK, None),
        },
        "sg_window_trend_buffer": {
            "off": (SG_ESTATE, "sg_window_trend_buffer: the trend is off (sg_set_trend)"),
            "was": (SG_OK, None),
            "flush": (SG_OK, None),
        },
        "sg_trend_entries": {
            "off": (SG_ESTATE, "sg_trend_entries: the trend is off (sg_set_trend)"),
            "flush": (SG_OK, None),
        },
        "sg_trend_stats_get": {
            "off": (SG_ESTATE, "sg_trend_stats_get: the trend is off (sg_set_trend)"),
            "flush": (SG_OK, None),
        },
        "sg_set_vanished": {
            "below_off": (SG_ESTATE, "sg_set_vanished: the trend is off (sg_set_trend)"),
            "bad": (SG_EINVAL, "sg_set_vanished: bad parameters"),
            "bad_flush": (SG_ESTATE, "sg_set_vanished while a flush is open"),
            "flush": (SG_ESTATE, "sg_set_vanished while a flush is open"),
        },
        "sg_window_vanished": {
            "off": (SG_ESTATE, "sg_window_vanished: the vanished list is off (sg_set_vanished)"),
            "was": (SG_ESTATE, "sg_window_vanished: the last read window was closed while the vanished list was off"),
            "flush": (SG_ESTATE, "sg_window_vanished while a flush is open"),
        },
        "sg_window_vanished_buffer": {
            "off": (SG_ESTATE, "sg_window_vanished_buffer: the vanished list is off (sg_set_vanished)"),
            "was": (SG_ESTATE, "sg_window_vanished_buffer: the window was closed while the vanished list was off"),
        },
        "sg_window_select_by": {
            "unknown_key": (SG_EINVAL, "selection: unknown key (by > SG_SEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "selection by a trend key: the trend is off (sg_set_trend)"),
        },
        "sg_flush_window_top_by": {
            "unknown_key": (SG_EINVAL, "selection: unknown key (by > SG_SEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "selection by a trend key: the trend is off (sg_set_trend)"),
        },
        "sg_window_nodes_top": {
            "below_off": (SG_ESTATE, "node selection: the node rollup is off (sg_set_nodes)"),
            "unknown_key": (SG_EINVAL, "node selection: unknown key (by > SG_NSEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "node selection by a trend key: the node trend is off (sg_set_node_trend)"),
            "was_below": (SG_ESTATE, "node selection: the window was closed while the node rollup was off"),
            "was": (SG_ESTATE, "node selection: the window was closed while the node trend was off"),
            "flush": (SG_ESTATE, "sg_window_nodes_top while a flush is open"),
        },
        "sg_window_nodes_select": {
            "below_off": (SG_ESTATE, "node selection: the node rollup is off (sg_set_nodes)"),
            "unknown_key": (SG_EINVAL, "node selection: unknown key (by > SG_NSEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "node selection by a trend key: the node trend is off (sg_set_node_trend)"),
            "was_below": (SG_ESTATE, "node selection: the window was closed while the node rollup was off"),
            "was": (SG_ESTATE, "node selection: the window was closed while the node trend was off"),
        },
    },
    "group": {
        "sg_set_group_trend": {
            "below_off": (SG_ESTATE, "sg_set_group_trend: the groups are off (sg_set_groups)"),
            "bad": (SG_EINVAL, "sg_set_group_trend: bad parameters"),
            "bad_flush": (SG_ESTATE, "sg_set_group_trend while a flush is open"),
            "flush": (SG_ESTATE, "sg_set_group_trend while a flush is open"),
        },
        "sg_window_group_trend": {
            "off": (SG_ESTATE, "sg_window_group_trend: the group trend is off (sg_set_group_trend)"),
            "was": (SG_ESTATE, "sg_window_group_trend: the last read window was closed while the group trend was off"),
            "beyond": (SG_EINVAL, "sg_window_group_trend: a group index beyond the window's group edges"),
            "flush": (SG_ESTATE, "sg_window_group_trend while a flush is open"),
        },
        "sg_window_group_trend_buffer": {
            "off": (SG_ESTATE, "sg_window_group_trend_buffer: the group trend is off (sg_set_group_trend)"),
            "was": (SG_ESTATE, "sg_window_group_trend_buffer: the window was closed while the group trend was off"),
        },
        "sg_group_trend_entries": {
            "off": (SG_ESTATE, "sg_group_trend_entries: the group trend is off (sg_set_group_trend)"),
            "flush": (SG_OK, None),
        },
        "sg_group_trend_stats_get": {
            "off": (SG_ESTATE, "sg_group_trend_stats_get: the group trend is off (sg_set_group_trend)"),
            "flush": (SG_OK, None),
        },
        "sg_set_group_vanished": {
            "below_off": (SG_ESTATE, "sg_set_group_vanished: the group trend is off (sg_set_group_trend)"),
            "bad": (SG_EINVAL, "sg_set_group_vanished: bad parameters"),
            "bad_flush": (SG_ESTATE, "sg_set_group_vanished while a flush is open"),
            "flush": (SG_ESTATE, "sg_set_group_vanished while a flush is open"),
        },
        "sg_window_group_vanished": {
            "off": (SG_ESTATE, "sg_window_group_vanished: the group vanished list is off (sg_set_group_vanished)"),
            "was": (SG_ESTATE, "sg_window_group_vanished: the last read window was closed while the group vanished list was off"),
            "flush": (SG_ESTATE, "sg_window_group_vanished while a flush is open"),
        },
        "sg_window_group_vanished_buffer": {
            "off": (SG_ESTATE, "sg_window_group_vanished_buffer: the group vanished list is off (sg_set_group_vanished)"),
            "was": (SG_ESTATE, "sg_window_group_vanished_buffer: the window was closed while the group vanished list was off"),
        },
        "sg_window_groups_top": {
            "below_off": (SG_ESTATE, "group selection: the groups are off (sg_set_groups)"),
            "unknown_key": (SG_EINVAL, "group selection: unknown key (by > SG_SEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "group selection by a trend key: the group trend is off (sg_set_group_trend)"),
            "was_below": (SG_ESTATE, "group selection: the window was closed while the groups were off"),
            "was": (SG_ESTATE, "group selection: the window was closed while the group trend was off"),
            "flush": (SG_ESTATE, "sg_window_groups_top while a flush is open"),
        },
        "sg_window_groups_select": {
            "below_off": (SG_ESTATE, "group selection: the groups are off (sg_set_groups)"),
            "unknown_key": (SG_EINVAL, "group selection: unknown key (by > SG_SEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "group selection by a trend key: the group trend is off (sg_set_group_trend)"),
            "was_below": (SG_ESTATE, "group selection: the window was closed while the groups were off"),
            "was": (SG_ESTATE, "group selection: the window was closed while the group trend was off"),
        },
        "sg_window_group_nodes_top": {
            "below_off": (SG_ESTATE, "workload selection: the workload rows are off (sg_set_group_nodes)"),
            "unknown_key": (SG_EINVAL, "workload selection: unknown key (by > SG_NSEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "workload selection by a trend key: the workload trend is off (sg_set_group_node_trend)"),
            "was_below": (SG_ESTATE, "workload selection: the window was closed while the workload rows were off"),
            "was": (SG_ESTATE, "workload selection: the window was closed while the workload trend was off"),
            "flush": (SG_ESTATE, "sg_window_group_nodes_top while a flush is open"),
        },
        "sg_window_group_nodes_select": {
            "below_off": (SG_ESTATE, "workload selection: the workload rows are off (sg_set_group_nodes)"),
            "unknown_key": (SG_EINVAL, "workload selection: unknown key (by > SG_NSEL_NEW)"),
            "kmax": (SG_EINVAL, None),
            "trend_key": (SG_ESTATE, "workload selection by a trend key: the workload trend is off (sg_set_group_node_trend)"),
            "was_below": (SG_ESTATE, "workload selection: the window was closed while the workload rows were off"),
            "was": (SG_ESTATE, "workload selection: the window was closed while the workload trend was off"),
        },
    },
}

KMAX1 = engine.SELECT_MAX_K + 1
SEL_PAST, NSEL_PAST = engine.SEL_BY["new"] + 1, engine.NSEL_BY["new"] + 1
LAT_DEV, IN_LAT_DEV = engine.SEL_BY["lat_dev"], engine.NSEL_BY["in_lat_dev"]
TTL = 8


class _Calls:
    """the entry points of one edge space and of the node space over it, called on the library itself: every method returns
    (name, (rc, sg_last_error after the call, or None when the call left the text as it was))"""

    def __init__(self, g, space):
        self.l, self.h, self.infix = g._l, g._h, "" if space == "edge" else "group_"

    def _do(self, name, *args):
        assert name in engine.EXPORTS
        assert self.l.sg_upsert_pod(self.h, 1, 0xFFFFFFFF) != SG_OK    # (a refusal that changes nothing, for its text)
        before = self.l.sg_last_error(self.h)
        assert before == b"node_id beyond max_known_nodes"
        rc = getattr(self.l, name)(self.h, *args)
        after = self.l.sg_last_error(self.h)
        return name, (rc, None if after == before else (after or b"").decode())

    def set_trend(self, **kw):
        p = engine.SgTrendParams(**{"struct_size": C.sizeof(engine.SgTrendParams), "ttl": TTL, **kw})
        return self._do(f"sg_set_{self.infix}trend", C.addressof(p))

    def set_vanished(self, **kw):
        p = engine.SgVanishedParams(**{"struct_size": C.sizeof(engine.SgVanishedParams), **kw})
        return self._do(f"sg_set_{self.infix}vanished", C.addressof(p))

    def trend(self, index=None):
        out = np.zeros(8, dtype=engine.TREND_DTYPE); n = C.c_size_t(0)
        name = f"sg_window_{self.infix}trend"
        if index is None:
            return self._do(name, None, 0, out.ctypes.data, len(out), C.byref(n))
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        return self._do(name, idx.ctypes.data, len(idx), out.ctypes.data, len(out), C.byref(n))

    def trend_buffer(self):
        p = C.c_void_p()
        return self._do(f"sg_window_{self.infix}trend_buffer", C.byref(p))

    def entries(self):
        out = np.zeros(8, dtype=engine.TREND_ENTRY_DTYPE); n = C.c_size_t(0)
        return self._do(f"sg_{self.infix}trend_entries", out.ctypes.data, len(out), C.byref(n))

    def stats(self):
        s = engine.SgTrendStats()
        return self._do(f"sg_{self.infix}trend_stats_get", C.addressof(s))

    def vanished(self):
        out = np.zeros(8, dtype=engine.VANISHED_DTYPE); n = C.c_size_t(0)
        return self._do(f"sg_window_{self.infix}vanished", out.ctypes.data, len(out), C.byref(n))

    def vanished_buffer(self):
        p = [C.c_void_p() for _ in range(2)]
        return self._do(f"sg_window_{self.infix}vanished_buffer", *(C.byref(x) for x in p))

    # the selections: the host form with room for 8 rows, the device form with no output but the count (never written: every call
    # of the device form here is refused before the launch)
    def _top(self, name, dtype, by, k):
        out, idx = np.zeros(8, dtype=dtype), np.zeros(8, dtype=np.uint32)
        n, m = C.c_size_t(0), C.c_size_t(0)
        return self._do(name, by, k, 0.0, out.ctypes.data, idx.ctypes.data, 8, C.byref(n), C.byref(m))

    def _select(self, name, by, k):
        d_n = C.c_uint64(0)
        return self._do(name, by, k, 0.0, None, None, 0, C.addressof(d_n), None)

    def edges_top(self, by, k=4):
        """sg_flush_window_top_by (it would close the open window: every call here is refused before that) or sg_window_groups_top"""
        if self.infix:
            return self._top("sg_window_groups_top", engine.GROUP_EDGE_DTYPE, by, k)
        out, idx = np.zeros(8, dtype=replay.EDGE_OUT_DTYPE), np.zeros(8, dtype=np.uint32)
        n, m = C.c_size_t(0), C.c_size_t(0)
        return self._do("sg_flush_window_top_by", 0, by, k, 0.0, out.ctypes.data, idx.ctypes.data, 8, C.byref(n), C.byref(m))

    def edges_select(self, by, k=4):
        return self._select("sg_window_groups_select" if self.infix else "sg_window_select_by", by, k)

    def nodes_top(self, by, k=4): return self._top(f"sg_window_{self.infix}nodes_top", engine.NODE_DTYPE, by, k)
    def nodes_select(self, by, k=4): return self._select(f"sg_window_{self.infix}nodes_select", by, k)


def _expect(space, state, *results):
    for name, got in results:
        assert got == EXPECT[space][name][state], (name, state)


def _ok(*results):
    for name, (rc, _text) in results:
        assert rc == SG_OK, name


@pytest.fixture(scope="module")
def stream():
    """four small windows over one topology of 1000 edges"""
    topo = replay.make_topology(120, 1000, seed=171)
    ev, labels = replay.make_events(topo, 48_000, seed=172, mixed=True, with_raw_outbound=True)
    return topo, labels, [ev[i * 12_000:(i + 1) * 12_000] for i in range(4)]


@pytest.mark.parametrize("space", ["edge", "group"])
def test_every_refusal_has_the_code_and_the_text(stream, space):
    topo, labels, wins = stream
    g = _engine(topo, labels, max_edges=4096, max_window_events=50_000)
    c = _Calls(g, space)
    group = space == "group"
    selections = lambda by, nby, k=4: (c.edges_top(by, k), c.edges_select(by, k), c.nodes_top(nby, k), c.nodes_select(nby, k))
    reads = lambda: (c.trend(), c.trend([0]), c.trend_buffer(), c.entries(), c.stats(), c.vanished(), c.vanished_buffer())

    # everything off: the stage below (the groups, the edge baseline, the rollup); a key one past the last and a k one past the
    # largest are refused before that
    _expect(space, "below_off", c.set_vanished(), c.nodes_top(0), c.nodes_select(0))
    if group:
        _expect(space, "below_off", c.set_trend(), c.set_trend(struct_size=4), c.edges_top(0), c.edges_select(0))
    _expect(space, "unknown_key", *selections(SEL_PAST, NSEL_PAST))
    _expect(space, "kmax", *selections(0, 0, KMAX1), *selections(SEL_PAST, NSEL_PAST, KMAX1))
    _expect(space, "off", *reads())
    _feed(g, wins[0]); g.flush_window()
    # the stage below on: bad parameters, a trend key with the baseline it reads off, the stage off, the window closed before
    if group:
        g.set_groups(); g.set_group_nodes()
    else:
        g.set_nodes()
    _expect(space, "bad", c.set_trend(struct_size=4), c.set_trend(shift=11))
    _expect(space, "trend_key", *selections(LAT_DEV, IN_LAT_DEV))
    _expect(space, "off", *reads())
    _expect(space, "was_below", c.nodes_top(0), c.nodes_select(0))
    if group:
        _expect(space, "was_below", c.edges_top(0), c.edges_select(0))
    _feed(g, wins[1]); g.flush_window()
    _expect(space, "off", *reads())
    # the baselines and the list on: the list's bad parameters, and the window closed while they were off
    _ok(c.set_trend())
    (g.set_group_node_trend if group else g.set_node_trend)(ttl=TTL)
    _expect(space, "bad", c.set_vanished(struct_size=4), c.set_vanished(silent_windows=TTL))
    _ok(c.set_vanished())
    _expect(space, "was", c.trend(), c.trend([0]), c.trend_buffer(), c.vanished(), c.vanished_buffer(), c.nodes_top(IN_LAT_DEV),
            c.nodes_select(IN_LAT_DEV))
    if group:
        _expect(space, "was", c.edges_top(LAT_DEV), c.edges_select(LAT_DEV))
    # a window closed with all of it on: every call answers, and an index equal to the window's row count is refused
    _feed(g, wins[2]); rows = g.flush_window()
    n = len(g.window_groups()) if group else len(rows)
    assert n > 8
    _ok(*reads(), c.trend([0, n - 1]), c.nodes_top(0), c.nodes_top(IN_LAT_DEV))
    if group:
        _ok(c.edges_top(0), c.edges_top(LAT_DEV))
    _expect(space, "beyond", c.trend([0, n]))
    # while a flush is open (sg_flush_begin leaves it open on the calling thread): the calls that look at it, and those that do not
    _feed(g, wins[3]); g.flush_begin()
    _expect(space, "flush", c.set_trend(), c.set_vanished(), c.vanished(), c.nodes_top(0), c.entries(), c.stats())
    _expect(space, "bad_flush", c.set_trend(struct_size=4), c.set_vanished(struct_size=4))
    if group:
        _expect(space, "flush", c.trend(), c.edges_top(0))
    else:
        _expect(space, "flush", c.trend(), c.trend_buffer())
    assert len(g.flush_end()) > 0
    _ok(*reads(), c.nodes_top(0))
