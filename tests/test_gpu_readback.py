"""The host readback of the opt-in window stages (K8 - K14), call by call: the indexed calls (sg_window_trend, sg_window_node_trend,
sg_window_rank, sg_window_node_incident, sg_window_row_group) against full[index], where full is the same call without an index (the
stage tests hold those full rows to their references), and the counted calls (sg_window_nodes, sg_window_incidents, sg_window_groups,
sg_window_group_perm, sg_window_vanished, sg_window_incident_tracks, sg_window_tracks_ended) against their own full answer — an empty
index, repeats in descending order, an index beyond the end, cap below the index' length, and an index longer than the device
staging, so that the gather goes in more than one piece (a last piece of one element included) or, for the two baselines, the
staging is grown from its 1024-row floor.

One small engine with every stage on.  Two windows are closed before anything is read, the second without two of the first's
chains: after a single window the vanished list and the ended list are empty, and "cap == n - 1" would check nothing."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.helpers import CLOCK, HostShim

pytestmark = pytest.mark.gpu

N_PODS = 48
GRP_STAGE = 65536                                                     # rows of sg_window_row_group's device staging
FILL = 0xA5


def _chain(lo, hi):
    return [(i, i + 1) for i in range(lo, hi - 1)]


def _close(topo, g, pairs):
    """one request per (src pod, dst pod) pair"""
    src, dst = (np.asarray(x) for x in zip(*pairs))
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = topo.pod_ips[dst]; e["status"] = np.where(np.arange(len(e)) % 3 == 0, 503, 200)
    e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = 1_000_000 + 37 * np.arange(len(e), dtype=np.uint64)
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    g.ingest_bulk(e)
    rows = g.flush_window().copy()
    assert len(rows) == len(e)
    return rows


@pytest.fixture(scope="module")
def eng():
    """(engine, E, N): every stage on; window 0 = five chains of 8 pods, window 1 (the one read) = three of them and a new one"""
    topo = replay.make_topology(N_PODS, 4 * N_PODS, seed=7, svcs=4)    # (only the pods and their ids are used)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=1 << 14, layers=2, max_labels=16, max_outbound_ips=64,
                            max_window_events=1 << 16, max_batch=1 << 14)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    g.set_trend(warmup=1); g.set_vanished()
    g.set_nodes(); g.set_node_trend(warmup=1); g.set_rank(iters=2); g.set_incidents(min_value=-float("inf")); g.set_tracks(quiet_windows=0)
    g.set_groups(); g.group_assign(np.arange(N_PODS), np.arange(N_PODS) % 5)
    _close(topo, g, sum((_chain(8 * c, 8 * c + 8) for c in range(5)), []))
    rows = _close(topo, g, sum((_chain(8 * c, 8 * c + 8) for c in (0, 1, 2, 5)), []))
    E, N = len(rows), len(g.window_nodes())
    assert E == 28 and N == 32
    return g, E, N


# name -> (the raw call, the wrapper, the row type, what the index runs over, the rows of the device staging (None: grown on demand))
def _indexed(g, E, N):
    l, ncap = g._l, g.window_buffers()[3]
    return {
        "window_trend": (l.sg_window_trend, g.window_trend, engine.TREND_DTYPE, E, None),
        "window_node_trend": (l.sg_window_node_trend, g.window_node_trend, engine.NODE_TREND_DTYPE, N, None),
        "window_rank": (l.sg_window_rank, g.window_rank, engine.RANK_DTYPE, N, ncap),
        "window_node_incident": (l.sg_window_node_incident, g.window_node_incident, np.dtype("<u4"), N, ncap),
        "window_row_group": (l.sg_window_row_group, g.window_row_group, np.dtype("<u4"), E, GRP_STAGE),
    }


INDEXED = ["window_trend", "window_node_trend", "window_rank", "window_node_incident", "window_row_group"]
COUNTED = ["window_nodes", "window_incidents", "window_groups", "window_group_perm", "window_vanished", "window_incident_tracks",
           "window_tracks_ended"]


def _counted(g):
    l = g._l
    return {
        "window_nodes": (l.sg_window_nodes, g.window_nodes, engine.NODE_DTYPE),
        "window_incidents": (l.sg_window_incidents, g.window_incidents, engine.INCIDENT_DTYPE),
        "window_groups": (l.sg_window_groups, g.window_groups, engine.GROUP_EDGE_DTYPE),
        "window_group_perm": (l.sg_window_group_perm, g.window_group_perm, np.dtype("<u4")),
        "window_vanished": (l.sg_window_vanished, g.window_vanished, engine.VANISHED_DTYPE),
        "window_incident_tracks": (l.sg_window_incident_tracks, g.window_incident_tracks, engine.TRACK_DTYPE),
        "window_tracks_ended": (l.sg_window_tracks_ended, g.window_tracks_ended, engine.TRACK_ENTRY_DTYPE),
    }


def _filled(n, dtype):
    """n rows of FILL bytes: what a call must leave where it writes nothing"""
    return np.frombuffer(bytes([FILL]) * (n * dtype.itemsize), dtype=dtype).copy()


def _raw(g, call, idx, dtype, cap=None, rows=None):
    """call(h, idx, len(idx), out, cap, &n) into `rows` FILL rows; (rc, out, n) with n preset to a value no call reports"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    rows = len(idx) if rows is None else rows
    out = _filled(rows, dtype)
    n = C.c_size_t(12345678)
    p = idx.ctypes.data if len(idx) else np.zeros(1, dtype=np.uint32).ctypes.data
    rc = call(g._h, p, len(idx), out.ctypes.data, len(idx) if cap is None else cap, C.byref(n))
    return rc, out, n.value


@pytest.fixture(scope="module")
def full(eng):
    """every indexed call's rows without an index: computed once, read only"""
    g, E, N = eng
    out = {}
    for name, (_, wrapper, dtype, count, _) in _indexed(g, E, N).items():
        out[name] = wrapper()
        assert len(out[name]) == count and out[name].dtype == dtype
        out[name].setflags(write=False)
    assert len(set(out["window_rank"]["rank"].tolist())) > 1 and len(set(out["window_row_group"].tolist())) > 1
    assert len(set(out["window_node_incident"].tolist())) == 4         # (the rows differ, so a wrong gather shows)
    return out


@pytest.mark.parametrize("name", INDEXED)
def test_an_empty_index(eng, name):
    g, E, N = eng
    call, wrapper, dtype, _, _ = _indexed(g, E, N)[name]
    rc, out, n = _raw(g, call, [], dtype, cap=4, rows=4)
    assert rc == engine.SG_OK and n == 0 and out.tobytes() == _filled(4, dtype).tobytes()
    assert len(wrapper(np.zeros(0, dtype=np.uint32))) == 0


@pytest.mark.parametrize("name", INDEXED)
def test_repeats_in_descending_order(eng, full, name):
    g, E, N = eng
    call, wrapper, dtype, count, _ = _indexed(g, E, N)[name]
    idx = np.repeat(np.arange(count - 1, -1, -1), 2)[:-1]             # count-1, count-1, count-2, ..., 1, 1, 0: an odd length
    assert wrapper(idx).tobytes() == full[name][idx].tobytes()
    rc, out, n = _raw(g, call, idx, dtype)
    assert rc == engine.SG_OK and n == len(idx) and out.tobytes() == full[name][idx].tobytes()


@pytest.mark.parametrize("name", INDEXED)
def test_an_index_one_past_the_end(eng, name):
    g, E, N = eng
    call, _, dtype, count, _ = _indexed(g, E, N)[name]
    rc, out, n = _raw(g, call, [0, count - 1, count], dtype)
    assert rc == engine.SG_EINVAL and b"beyond the window's" in g._l.sg_last_error(g._h)
    assert out.tobytes() == _filled(3, dtype).tobytes()
    assert n == 12345678                                              # (the index is checked before anything is written)
    rc, out, n = _raw(g, call, [count - 1], dtype)                    # the last one is in range
    assert rc == engine.SG_OK and n == 1


@pytest.mark.parametrize("name", INDEXED)
def test_cap_below_the_index_length(eng, full, name):
    g, E, N = eng
    call, _, dtype, count, _ = _indexed(g, E, N)[name]
    idx = np.array([3, count - 1, 0, 3, 7, 1, 2], dtype=np.uint32)
    rc, out, n = _raw(g, call, idx, dtype, cap=4)
    assert rc == engine.SG_OK and n == len(idx)
    assert out[:4].tobytes() == full[name][idx[:4]].tobytes() and out[4:].tobytes() == _filled(3, dtype).tobytes()
    rc, out, n = _raw(g, call, idx, dtype, cap=0)
    assert rc == engine.SG_OK and n == len(idx) and out.tobytes() == _filled(len(idx), dtype).tobytes()
    m = C.c_size_t(0)                                                 # no output at all: the count alone
    assert call(g._h, idx.ctypes.data, len(idx), None, 0, C.byref(m)) == engine.SG_OK and m.value == len(idx)


# (the piece arithmetic: one element more than the staging is the smallest index whose last piece has one element; three more, and two
# stagings and one: a last piece that is neither full nor one, and more than two pieces)
@pytest.mark.parametrize("extra", [1, 3, "two stagings and one"])
@pytest.mark.parametrize("name", ["window_rank", "window_node_incident", "window_row_group"])
def test_an_index_longer_than_the_staging_goes_in_pieces(eng, full, name, extra):
    g, E, N = eng
    call, wrapper, dtype, count, stage = _indexed(g, E, N)[name]
    assert stage >= count                                             # (the node capacity, or 65536 rows)
    n_index = 2 * stage + 1 if extra == "two stagings and one" else stage + extra
    k = np.arange(n_index, dtype=np.uint64)
    idx = ((k * 7 + k // stage) % count).astype(np.uint32)            # repeats; the pieces start at different rows
    idx[-1] = count - 1
    rc, out, n = _raw(g, call, idx, dtype)
    assert rc == engine.SG_OK and n == n_index and out.tobytes() == full[name][idx].tobytes()
    rc, out, n = _raw(g, call, idx, dtype, cap=stage + 1)             # the cut falls into the second piece: one element of it
    assert rc == engine.SG_OK and n == n_index
    assert out[: stage + 1].tobytes() == full[name][idx[: stage + 1]].tobytes()
    assert out[stage + 1:].tobytes() == _filled(n_index - stage - 1, dtype).tobytes()


@pytest.mark.parametrize("name", ["window_trend", "window_node_trend"])
def test_the_baselines_staging_grows_and_is_kept(eng, full, name):
    """5 entries (the staging's floor, 1024 rows), 1025 (it is grown), 5 again, in the same engine"""
    g, E, N = eng
    call, wrapper, dtype, count, _ = _indexed(g, E, N)[name]
    for n_index in (5, 1025, 5, 1024, 1026):
        k = np.arange(n_index, dtype=np.uint64)
        idx = ((k * 5 + 3) % count).astype(np.uint32)
        idx[-1] = count - 1
        rc, out, n = _raw(g, call, idx, dtype)
        assert rc == engine.SG_OK and n == n_index and out.tobytes() == full[name][idx].tobytes(), n_index
    assert wrapper().tobytes() == full[name].tobytes()


@pytest.mark.parametrize("name", COUNTED)
def test_a_counted_call_with_no_room_and_with_one_row_too_few(eng, name):
    g, E, N = eng
    call, wrapper, dtype = _counted(g)[name]
    want = wrapper()
    assert len(want) >= 2 and want.dtype == dtype, "the window must leave this call at least two rows"
    n = C.c_size_t(12345678)
    assert call(g._h, None, 0, C.byref(n)) == engine.SG_OK and n.value == len(want)
    out = _filled(len(want), dtype)
    n = C.c_size_t(12345678)
    assert call(g._h, out.ctypes.data, len(want) - 1, C.byref(n)) == engine.SG_OK and n.value == len(want)
    assert out[:-1].tobytes() == want[:-1].tobytes() and out[-1:].tobytes() == _filled(1, dtype).tobytes()
    out = _filled(len(want), dtype)                                   # room for none, with somewhere to write: nothing written
    assert call(g._h, out.ctypes.data, 0, C.byref(n)) == engine.SG_OK and n.value == len(want)
    assert out.tobytes() == _filled(len(want), dtype).tobytes()


def test_every_stage_block_keeps_its_layout_across_the_slots():
    """The stage blocks' layout (sg_plan.hpp) seen through the *_buffer calls: three windows in flight, every stage on, one window
    run per slot.  Inside a slot the pieces lie the same distance apart in all three slots, the slots lie one constant stride
    apart, every distance is a multiple of 256 bytes, and every piece has room for what this engine's capacities can put into it
    before the next piece (or the next slot) begins.  Prints the distances (one "layout ..." line per stage).

    max_labels = max_outbound_ips = 0 is the smallest configuration sg_create accepts (the outbound-IP space keeps one id): 5 node keys."""
    import torch
    in_flight, mk, me = 3, 4, 8
    topo = replay.make_topology(2, 2, seed=7, svcs=1)                  # (only the two pods and their ids are used)
    g = engine.ServiceGraph(max_known_nodes=mk, max_edges=me, layers=2, max_labels=0, max_outbound_ips=0, max_window_events=1 << 10,
                            max_batch=1 << 10, windows_in_flight=in_flight)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    g.set_trend(warmup=1); g.set_vanished()
    g.set_nodes(); g.set_node_trend(warmup=1); g.set_rank(iters=2); g.set_incidents(min_value=-float("inf")); g.set_tracks(quiet_windows=0)
    g.set_groups(); g.group_assign(np.arange(2), np.zeros(2, dtype=np.uint32))
    ncap = g.window_buffers()[3]
    assert ncap == mk + 0 + 1
    e = np.zeros(5, dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[0]; e["daddr"] = topo.pod_ips[1]; e["status"] = 200; e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = 1_000_000 + 37 * np.arange(len(e), dtype=np.uint64)
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    dev = torch.from_numpy(e.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    one = lambda f: (lambda: (f(),))                                  # noqa: E731  (a call that returns one pointer)
    sz = lambda d: d.itemsize                                         # noqa: E731
    vanished_rows = 2 * me                                            # max_rows: min(65536, max_entries), max_entries: 2 x max_edges
    # stage -> (the *_buffer call, the bytes each of its pieces must hold at this engine's capacities, in the call's order)
    stages = {
        "trend": (one(g.trend_buffer), [me * sz(engine.TREND_DTYPE)]),
        "vanished": (g.vanished_buffer, [vanished_rows * sz(engine.VANISHED_DTYPE), 8]),
        "nodes": (g.nodes_buffer, [ncap * sz(engine.NODE_DTYPE), 8]),
        "node_trend": (one(g.node_trend_buffer), [ncap * sz(engine.NODE_TREND_DTYPE)]),
        "rank": (one(g.rank_buffer), [ncap * sz(engine.RANK_DTYPE)]),
        "incidents": (g.window_incidents_buffer, [ncap * sz(engine.INCIDENT_DTYPE), 8, ncap * 4]),                # rows, count, node_incident
        "tracks": (g.window_tracks_buffer, [ncap * sz(engine.TRACK_DTYPE), ncap * sz(engine.TRACK_ENTRY_DTYPE), 8]),   # tracks, ended, ended_count
        "groups": (g.window_groups_buffer, [me * sz(engine.GROUP_EDGE_DTYPE), 8, me * 4, me * 4]),              # edges, count, row_group, perm
    }
    seen = {name: [] for name in stages}
    for _ in range(in_flight):
        g.ingest_device(dev.data_ptr(), len(e), 0)
        g.window_run(0)
        for name, (call, _) in stages.items():
            seen[name].append(tuple(int(p) for p in call()))
    torch.cuda.synchronize()
    for name, (_, need) in stages.items():
        slots = sorted(seen[name])
        assert len(set(slots)) == in_flight, name                         # every slot has buffers of its own
        inner = [[p - s[0] for p in s] for s in slots]
        strides = [b[0] - a[0] for a, b in zip(slots, slots[1:])]
        print("layout", name, "inside a slot", inner[0], "slot stride", strides[0])
        assert inner[0] == inner[1] == inner[2], (name, inner)            # the same distances in all three slots
        assert strides[0] == strides[1], (name, strides)                  # a constant stride
        assert all(x % 256 == 0 for x in inner[0] + strides), (name, inner[0], strides)
        order = sorted(range(len(need)), key=lambda i: inner[0][i])       # (the call's order need not be the block's)
        for a, b in zip(order, order[1:] + [None]):
            room = (inner[0][b] if b is not None else strides[0]) - inner[0][a]
            assert room >= need[a], (name, a, room, need[a])             # (the last piece: up to the next slot, so none lies beyond its slot)
