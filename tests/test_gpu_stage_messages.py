"""The engine's own sg_last_error texts of the ranking and the incidents, over the nodes (K11, K12) and over the workloads (K17, K18):
the return code and the exact text of every refusal these entry points have.  The other suites check the codes; the front-end tests
script the texts through a stand-in library.  EXPECT is a literal table: the calls go to the C functions directly, so that no
Python-side check or helper call answers in the engine's place."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.engine import SG_EINVAL, SG_ESTATE, SG_OK
from tests.gpu_scaffold import _engine, _feed
from tests.traces import churn  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

#: call -> state -> (return code, sg_last_error).  States: rollup_off (the space's rollup off), bad (bad parameters), trend_key (a
#: trend key with the space's edge baseline off), off (the stage off), was (a window closed while the stage was off), beyond (an
#: index equal to the window's row count), flush (between sg_flush_begin and sg_flush_end)
EXPECT = {
    "node": {
        "sg_set_rank": {
            "rollup_off": (SG_ESTATE, "sg_set_rank: the node rollup is off (sg_set_nodes)"),
            "bad": (SG_EINVAL, "sg_set_rank: bad parameters"),
            "flush": (SG_ESTATE, "sg_set_rank while a flush is open"),
        },
        "sg_set_incidents": {
            "rollup_off": (SG_ESTATE, "sg_set_incidents: the node rollup is off (sg_set_nodes)"),
            "bad": (SG_EINVAL, "sg_set_incidents: bad parameters"),
            "trend_key": (SG_ESTATE, "sg_set_incidents by a trend key: the trend is off (sg_set_trend)"),
            "flush": (SG_ESTATE, "sg_set_incidents while a flush is open"),
        },
        "sg_window_rank": {
            "off": (SG_ESTATE, "sg_window_rank: the ranking is off (sg_set_rank)"),
            "was": (SG_ESTATE, "sg_window_rank: the last read window was closed while the ranking was off"),
            "beyond": (SG_EINVAL, "sg_window_rank: a node index beyond the window's nodes"),
            "flush": (SG_ESTATE, "sg_window_rank while a flush is open"),
        },
        "sg_window_rank_buffer": {
            "off": (SG_ESTATE, "sg_window_rank_buffer: the ranking is off (sg_set_rank)"),
            "was": (SG_ESTATE, "sg_window_rank_buffer: the window was closed while the ranking was off"),
        },
        "sg_window_rank_top": {
            "rollup_off": (SG_ESTATE, "rank selection: the node rollup is off (sg_set_nodes)"),
            "off": (SG_ESTATE, "rank selection: the ranking is off (sg_set_rank)"),
            "was": (SG_ESTATE, "rank selection: the window was closed while the ranking was off"),
            "flush": (SG_ESTATE, "sg_window_rank_top while a flush is open"),
        },
        "sg_window_rank_select": {
            "rollup_off": (SG_ESTATE, "rank selection: the node rollup is off (sg_set_nodes)"),
            "off": (SG_ESTATE, "rank selection: the ranking is off (sg_set_rank)"),
            "was": (SG_ESTATE, "rank selection: the window was closed while the ranking was off"),
        },
        "sg_window_incidents": {
            "off": (SG_ESTATE, "sg_window_incidents: the incidents are off (sg_set_incidents)"),
            "was": (SG_ESTATE, "sg_window_incidents: the last read window was closed while the incidents were off"),
            "flush": (SG_ESTATE, "sg_window_incidents while a flush is open"),
        },
        "sg_window_node_incident": {
            "off": (SG_ESTATE, "sg_window_node_incident: the incidents are off (sg_set_incidents)"),
            "was": (SG_ESTATE, "sg_window_node_incident: the last read window was closed while the incidents were off"),
            "beyond": (SG_EINVAL, "sg_window_node_incident: a node index beyond the window's nodes"),
            "flush": (SG_ESTATE, "sg_window_node_incident while a flush is open"),
        },
        "sg_window_incidents_buffer": {
            "off": (SG_ESTATE, "sg_window_incidents_buffer: the incidents are off (sg_set_incidents)"),
            "was": (SG_ESTATE, "sg_window_incidents_buffer: the window was closed while the incidents were off"),
        },
    },
    "workload": {
        "sg_set_group_rank": {
            "rollup_off": (SG_ESTATE, "sg_set_group_rank: the workload rows are off (sg_set_group_nodes)"),
            "bad": (SG_EINVAL, "sg_set_group_rank: bad parameters"),
            "flush": (SG_ESTATE, "sg_set_group_rank while a flush is open"),
        },
        "sg_set_group_incidents": {
            "rollup_off": (SG_ESTATE, "sg_set_group_incidents: the workload rows are off (sg_set_group_nodes)"),
            "bad": (SG_EINVAL, "sg_set_group_incidents: bad parameters"),
            "trend_key": (SG_ESTATE, "sg_set_group_incidents by a trend key: the group trend is off (sg_set_group_trend)"),
            "flush": (SG_ESTATE, "sg_set_group_incidents while a flush is open"),
        },
        "sg_window_group_rank": {
            "off": (SG_ESTATE, "sg_window_group_rank: the workload ranking is off (sg_set_group_rank)"),
            "was": (SG_ESTATE, "sg_window_group_rank: the last read window was closed while the workload ranking was off"),
            "beyond": (SG_EINVAL, "sg_window_group_rank: a node index beyond the window's workload rows"),
            "flush": (SG_ESTATE, "sg_window_group_rank while a flush is open"),
        },
        "sg_window_group_rank_buffer": {
            "off": (SG_ESTATE, "sg_window_group_rank_buffer: the workload ranking is off (sg_set_group_rank)"),
            "was": (SG_ESTATE, "sg_window_group_rank_buffer: the window was closed while the workload ranking was off"),
        },
        "sg_window_group_rank_top": {
            "rollup_off": (SG_ESTATE, "workload rank selection: the workload rows are off (sg_set_group_nodes)"),
            "off": (SG_ESTATE, "workload rank selection: the workload ranking is off (sg_set_group_rank)"),
            "was": (SG_ESTATE, "workload rank selection: the window was closed while the workload ranking was off"),
            "flush": (SG_ESTATE, "sg_window_group_rank_top while a flush is open"),
        },
        "sg_window_group_rank_select": {
            "rollup_off": (SG_ESTATE, "workload rank selection: the workload rows are off (sg_set_group_nodes)"),
            "off": (SG_ESTATE, "workload rank selection: the workload ranking is off (sg_set_group_rank)"),
            "was": (SG_ESTATE, "workload rank selection: the window was closed while the workload ranking was off"),
        },
        "sg_window_group_incidents": {
            "off": (SG_ESTATE, "sg_window_group_incidents: the workload incidents are off (sg_set_group_incidents)"),
            "was": (SG_ESTATE, "sg_window_group_incidents: the last read window was closed while the workload incidents were off"),
            "flush": (SG_ESTATE, "sg_window_group_incidents while a flush is open"),
        },
        "sg_window_group_node_incident": {
            "off": (SG_ESTATE, "sg_window_group_node_incident: the workload incidents are off (sg_set_group_incidents)"),
            "was": (SG_ESTATE, "sg_window_group_node_incident: the last read window was closed while the workload incidents were off"),
            "beyond": (SG_EINVAL, "sg_window_group_node_incident: a node index beyond the window's workload rows"),
            "flush": (SG_ESTATE, "sg_window_group_node_incident while a flush is open"),
        },
        "sg_window_group_incidents_buffer": {
            "off": (SG_ESTATE, "sg_window_group_incidents_buffer: the workload incidents are off (sg_set_group_incidents)"),
            "was": (SG_ESTATE, "sg_window_group_incidents_buffer: the window was closed while the workload incidents were off"),
        },
    },
}


class _Calls:
    """the nine entry points of one space, called on the library itself: every method returns (rc, sg_last_error after the call)"""

    def __init__(self, g, space):
        self.l, self.h, self.infix = g._l, g._h, "" if space == "node" else "group_"

    def _do(self, which, *args):
        name = f"sg_set_{self.infix}{which[4:]}" if which.startswith("set_") else f"sg_window_{self.infix}{which}"
        assert name in engine.EXPORTS
        rc = getattr(self.l, name)(self.h, *args)
        return name, (rc, (self.l.sg_last_error(self.h) or b"").decode())

    def set_rank(self, **kw):
        p = engine.SgRankParams(**{"struct_size": C.sizeof(engine.SgRankParams), **kw})
        return self._do("set_rank", C.addressof(p))

    def set_incidents(self, **kw):
        p = engine.SgIncidentParams(**{"struct_size": C.sizeof(engine.SgIncidentParams), **kw})
        return self._do("set_incidents", C.addressof(p))

    def _indexed(self, which, dtype, index):
        out = np.zeros(8, dtype=dtype); n = C.c_size_t(0)
        if index is None:
            return self._do(which, None, 0, out.ctypes.data, len(out), C.byref(n))
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        return self._do(which, idx.ctypes.data, len(idx), out.ctypes.data, len(out), C.byref(n))

    def rank(self, index=None): return self._indexed("rank", engine.RANK_DTYPE, index)
    def node_incident(self, index=None): return self._indexed("node_incident", np.dtype("<u4"), index)

    def incidents(self):
        out = np.zeros(8, dtype=engine.INCIDENT_DTYPE); n = C.c_size_t(0)
        return self._do("incidents", out.ctypes.data, len(out), C.byref(n))

    def rank_buffer(self):
        p = C.c_void_p()
        return self._do("rank_buffer", C.byref(p))

    def incidents_buffer(self):
        p = [C.c_void_p() for _ in range(3)]
        return self._do("incidents_buffer", *(C.byref(x) for x in p))

    def rank_top(self):
        out, rk, idx = np.zeros(8, dtype=engine.NODE_DTYPE), np.zeros(8, dtype=engine.RANK_DTYPE), np.zeros(8, dtype=np.uint32)
        n, m = C.c_size_t(0), C.c_size_t(0)
        return self._do("rank_top", 4, 0.0, out.ctypes.data, rk.ctypes.data, idx.ctypes.data, 8, C.byref(n), C.byref(m))

    def rank_select(self):
        d_n = C.c_uint64(0)                                           # (never written: every call here is refused before the launch)
        return self._do("rank_select", 4, 0.0, None, None, 0, C.addressof(d_n), None)


def _expect(space, state, *results):
    for name, got in results:
        assert got == EXPECT[space][name][state], (name, state)


@pytest.mark.parametrize("space", ["node", "workload"])
def test_every_refusal_has_the_code_and_the_text(churn, space):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    c = _Calls(g, space)
    roll_on = g.set_nodes if space == "node" else (lambda: (g.set_groups(), g.set_group_nodes()))
    rows_of = g.window_nodes if space == "node" else g.window_group_nodes
    lat_dev = engine.SEL_BY["lat_dev"]

    # the rollup of the space off
    _expect(space, "rollup_off", c.set_rank(), c.set_incidents(), c.rank_top(), c.rank_select())
    roll_on()
    # bad parameters; a trend key while the edge baseline of the space is off
    _expect(space, "bad", c.set_rank(struct_size=4), c.set_rank(iters=65), c.set_incidents(struct_size=4), c.set_incidents(by=lat_dev + 2))
    _expect(space, "trend_key", c.set_incidents(by=lat_dev))
    # the stage off: every read, every *_buffer call, the two selections
    off = lambda: (c.rank(), c.rank([0]), c.rank_buffer(), c.rank_top(), c.rank_select(), c.incidents(), c.node_incident(),
                   c.node_incident([0]), c.incidents_buffer())
    _expect(space, "off", *off())
    _feed(g, wins[0]); g.flush_window()
    _expect(space, "off", *off())
    # a window closed while the stage was off
    assert c.set_rank()[1][0] == SG_OK and c.set_incidents()[1][0] == SG_OK
    _expect(space, "was", c.rank(), c.rank([0]), c.rank_buffer(), c.rank_top(), c.rank_select(), c.incidents(), c.node_incident(),
            c.node_incident([0]), c.incidents_buffer())
    # a window closed with both on: every call answers, and an index equal to the window's row count is refused
    _feed(g, wins[1]); g.flush_window()
    n = len(rows_of())
    assert n > 8
    for _, (rc, _text) in (c.rank(), c.rank([n - 1]), c.rank_buffer(), c.incidents(), c.node_incident(), c.node_incident([0, n - 1]),
                           c.incidents_buffer(), c.rank_top()):
        assert rc == SG_OK
    _expect(space, "beyond", c.rank([0, n]), c.node_incident([n]))
    # while a flush is open (sg_flush_begin leaves it open on the calling thread; the *_buffer and *_select calls do not look at it)
    _feed(g, wins[2]); g.flush_begin()
    _expect(space, "flush", c.set_rank(), c.set_incidents(), c.rank(), c.rank_top(), c.incidents(), c.node_incident())
    assert len(g.flush_end()) > 0
    for _, (rc, _text) in (c.rank(), c.incidents(), c.node_incident()):
        assert rc == SG_OK
