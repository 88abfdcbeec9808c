"""K14, the groups (sg_set_groups / sg_group_assign / sg_window_groups / sg_window_row_group / sg_window_group_perm /
sg_window_groups_buffer): the group edges, row_group and perm of every window against the pure-Python reference tests/group_ref.py
run on the same window's rows — byte for byte, every field is an integer or a max of float bits — on every close path, under maps
that change between windows and between slots, an engine with it against a twin without it, and constructed windows at the edges of
the radix sort (4096-position tiles, 2048-position fold chunks, odd and even pass counts, 32- and 64-bit keys)."""
import numpy as np
import pytest

from alaz_amd import engine, replay
from tests.gpu_scaffold import _d2h, _engine, _feed, _grouped, _hip, _map, _pairs, _path, _pods_engine, _rc
from tests.group_ref import group_ref
from tests.nodes_ref import nodes_ref
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

NO = engine.NO_GROUP
ML = 256                                                              # max_labels of _engine
TILE, CHUNK = 4096, 2048


def _check(g, rows, gmap, mg, mk, ml=ML, got=None, rng=None):
    """the last read window's group edges, row_group and perm (or `got` = the three) against the reference over `rows`"""
    want, wrg, wperm = group_ref(rows, gmap, mg, mk, ml)
    ge, rg, perm = (g.window_groups(), g.window_row_group(), g.window_group_perm()) if got is None else got
    assert perm.tobytes() == wperm.tobytes()
    assert rg.tobytes() == wrg.tobytes()
    assert len(ge) == len(want)
    for f in ge.dtype.names:
        assert ge[f].tobytes() == want[f].tobytes(), f
    if got is None and len(rows):
        idx = (rng or np.random.default_rng(len(rows))).integers(0, len(rows), 41).astype(np.uint32)
        assert g.window_row_group(idx).tolist() == wrg[idx].tolist()
        assert _rc(g.window_row_group, np.array([len(rows)], np.uint32)) == engine.SG_EINVAL
    return ge


@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
def test_every_window_of_the_churn_is_exact(churn, kind):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, kind)
    shrink = set()
    for w in wins:
        _feed(g, w)
        rows = g.flush_window().copy()
        ge = _check(g, rows, gmap, mk, mk)
        shrink.add(len(ge) < len(rows))
        assert (len(ge) == len(rows)) == (kind == "none")
    assert shrink == {kind != "none"}


@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
def test_warm_delta_and_cold_windows(warm_stream, kind):
    topo, labels, wins = warm_stream
    g, gmap, mk = _grouped(topo, labels, kind, max_window_events=700_000)
    seen = []
    for w in wins:
        _feed(g, w)
        s0 = g.stats()
        rows = g.flush_window().copy()
        seen.append(_path(s0, g.stats()))
        _check(g, rows, gmap, mk, mk)
    assert {"cold", "warm", "delta"} <= set(seen), seen


# ---- constructed windows: pod-to-pod events only, one request per (src pod, dst pod) pair ------------------------------------------


def _close(topo, g, src, dst):
    src, dst = np.asarray(src), np.asarray(dst)
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = topo.pod_ips[dst]; e["status"] = np.where(np.arange(len(e)) % 3 == 0, 503, 200)
    e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = 1_000_000 + 37 * np.arange(len(e), dtype=np.uint64)
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    if len(e):
        g.ingest_bulk(e)
    rows = g.flush_window().copy()
    assert len(rows) == len(e)
    return rows


# max_known, max_groups -> GK, bits, passes: 382 -> 9 bits, 3 passes (u32); 4000 + 4080 -> 13 bits, 4 passes (u32);
# 40 000 + 40 080 -> 17 bits, 5 passes (u64 keys)
SORTS = [(None, 0), (4000, 0), (40_000, 0)]


@pytest.fixture(scope="module", params=SORTS, ids=["3-pass", "4-pass", "5-pass-u64"])
def pods(request):
    mk, mg = request.param
    topo, g, mk = _pods_engine(mk, mg)
    return topo, g, mk, mg or mk


@pytest.mark.parametrize("E", [0, 1, TILE, TILE + 1, 3 * TILE + 1])
def test_window_sizes_at_the_tile_edges(pods, E):
    topo, g, mk, mg = pods
    gmap = _map("blocks", mk, topo.n_pods)
    g.set_groups(max_groups=mg); g.group_assign(np.arange(mk), gmap)
    rows = _close(topo, g, *_pairs(topo.n_pods, E, 100 + E))
    ge = _check(g, rows, gmap, mg, mk, 16)
    assert int(ge["edges"].sum()) == E and (E == 0 or len(ge) < E or E == 1)


def test_one_key_for_every_row_and_a_key_for_each(pods):
    topo, g, mk, mg = pods
    E = 2 * CHUNK + 904
    src, dst = _pairs(topo.n_pods, E, 5)
    g.set_groups(max_groups=mg); g.group_assign(np.arange(topo.n_pods), 3)      # every pod in workload 3: one run across three chunks
    gmap = np.full(mk, NO, np.uint32); gmap[:topo.n_pods] = 3
    ge = _check(g, _close(topo, g, src, dst), gmap, mg, mk, 16)
    assert len(ge) == 1 and ge["edges"][0] == E > CHUNK and ge["first"][0] == 0 and ge["from_nodes"][0] == len(set(src.tolist()))
    assert g.window_group_perm().tolist() == list(range(E))
    g.set_groups(max_groups=mg)                                       # the map starts over: nothing grouped, every row its own key
    ge = _check(g, _close(topo, g, src, dst), np.full(mk, NO, np.uint32), mg, mk, 16)
    assert len(ge) == E and ge["first"].tolist() == list(range(E)) == g.window_row_group().tolist()


def test_a_group_scattered_over_every_tile(pods):
    topo, g, mk, mg = pods
    gmap = np.full(mk, NO, np.uint32)
    far = np.arange(0, topo.n_pods, 13)                              # pods 0, 13, 26, ...: their rows lie all over the canonical order
    gmap[far] = 1
    gmap[np.arange(5, topo.n_pods, 29)] = 0
    g.set_groups(max_groups=mg); g.group_assign(np.arange(mk), gmap)
    rows = _close(topo, g, *_pairs(topo.n_pods, 3 * TILE + 1, 77))
    ge = _check(g, rows, gmap, mg, mk, 16)
    inside = ge[(ge["from_ref"] == ((3 << 30) | 1)) & (ge["to_ref"] == ((3 << 30) | 1))]
    assert len(inside) == 1 and inside["edges"][0] > 1
    perm = g.window_group_perm()
    mine = perm[inside["first"][0]:inside["first"][0] + inside["edges"][0]]
    assert (np.diff(mine.astype(np.int64)) > 0).all() and len({int(j) // TILE for j in mine}) >= 3      # stable, and from every full tile


def test_digits_of_0_and_255_in_every_pass():
    """GK = 65 536: 16 + 16 key bits, four passes; the workloads 0x0000, 0x00FF and 0xFF00 give every pass digits of 0 and of 255"""
    topo, g, mk = _pods_engine(64, n_pods=12, max_outbound_ips=16)
    ncap = g.window_buffers()[3]
    mg = 65536 - ncap
    assert 0xFF00 < mg
    gmap = np.full(mk, NO, np.uint32)
    gmap[:12] = np.array([0x0000, 0x00FF, 0xFF00])[np.arange(12) % 3]
    g.set_groups(max_groups=mg); g.group_assign(np.arange(mk), gmap)
    src, dst = _pairs(12, 132, 3)
    rows = _close(topo, g, src, dst)
    ge = _check(g, rows, gmap, mg, mk, 16)
    assert len(ge) == 9 and sorted(set(ge["from_ref"].tolist())) == [(3 << 30) | x for x in (0, 0xFF, 0xFF00)]
    for shift in (0, 8, 16, 24):                                      # the reference's keys: both digits in every pass
        key = ((ge["from_ref"].astype(np.uint64) & np.uint64(0xFFFF)) << np.uint64(16)) | (ge["to_ref"].astype(np.uint64) & np.uint64(0xFFFF))
        assert set(((key >> np.uint64(shift)) & np.uint64(255)).tolist()) == {0, 255}


# ---- the map over time ------------------------------------------------------------------------------------------------------------
def test_the_map_changes_between_windows(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    mk = topo.n_nodes + 8
    g.set_groups(max_groups=50)
    gmap = np.full(mk, NO, np.uint32)
    rng = np.random.default_rng(14)
    for i, w in enumerate(wins[:6]):
        ids = rng.integers(0, topo.n_pods, 60).astype(np.uint32)
        gs = np.where(rng.random(60) < 0.2, NO, rng.integers(0, 50, 60)).astype(np.uint32)
        g.group_assign(ids, gs)
        for k, v in zip(ids, gs):                                     # in call order: a later pair of one call wins
            gmap[k] = v
        _feed(g, w)
        _check(g, g.flush_window().copy(), gmap, 50, mk)
    assert _rc(g.group_assign, [mk], [0]) == engine.SG_EINVAL and _rc(g.group_assign, [0, 1], [3, 50]) == engine.SG_EINVAL
    _feed(g, wins[6])
    _check(g, g.flush_window().copy(), gmap, 50, mk)                   # a refused call applied nothing, not even its good pair


def test_window_run_in_flight_under_a_changing_map(churn):
    """sg_window_run with three windows in flight: a map change made between two closes is seen by the later window only, though the
    earlier one may still be running on another slot; read through sg_window_groups_buffer after the round was enqueued"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=3), _engine(topo, labels)
    mk = topo.n_nodes + 8
    g.set_groups()
    gmap = np.full(mk, NO, np.uint32)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        rows = one.flush_window().copy()
        lo = 30 * i
        g.group_assign(np.arange(lo, lo + 40), np.arange(lo, lo + 40) // (3 + i % 4))
        gmap[lo:lo + 40] = np.arange(lo, lo + 40) // (3 + i % 4)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((rows, gmap.copy(), g.window_groups_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for rows, m, (ep, cp, rp, pp) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                got = (_d2h(hip, ep, cnt, engine.GROUP_EDGE_DTYPE), _d2h(hip, rp, len(rows), np.uint32), _d2h(hip, pp, len(rows), np.uint32))
                _check(g, rows, m, mk, mk, got=got)
                sizes.append(cnt)
            pending = []
    assert len(sizes) == 9 and len(set(sizes)) > 3


def test_every_close_path_gives_the_same_group_edges(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    twin = _engine(topo, labels)
    for i, w in enumerate(wins[:7]):
        _feed(g, w); _feed(twin, w)
        full = twin.flush_window().copy()
        if i == 0:
            g.flush_begin()
            assert _rc(g.window_groups) == engine.SG_ESTATE and _rc(g.window_row_group) == engine.SG_ESTATE      # a flush is open
            assert _rc(g.window_group_perm) == engine.SG_ESTATE
            assert _rc(g.set_groups) == engine.SG_ESTATE and _rc(g.set_groups, None) == engine.SG_ESTATE
            rows = g.flush_end().copy()
        elif i == 1:
            rows = g.flush_window_view().copy()
        elif i == 2:
            g.flush_begin()
            rows = g.flush_end_view().copy()
        elif i == 3:
            sel, idx, n_edges = g.flush_window_top(3)
            assert n_edges == len(full)
            rows = full
        elif i == 4:
            g.window_run()
            rows = g.window_read().copy()
        elif i == 5:
            g.window_close(); g.window_features()
            for l in range(2):
                g.window_layer(l)
            g.window_score()
            rows = g.window_read().copy()
            g.window_reset()
        else:
            rows = g.flush_window().copy()
        assert rows.tobytes() == full.tobytes()
        _check(g, rows, gmap, mk, mk)


def test_a_twin_without_it_is_unchanged(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(shift=3, warmup=2, ttl=4); x.set_vanished(silent_windows=1, min_seen=1)
        x.set_node_trend(shift=3, warmup=2, ttl=3, max_entries=700); x.set_rank(iters=3)
        x.set_incidents(min_value=0.5); x.set_tracks(quiet_windows=1)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    g.set_groups(); g.group_assign(np.arange(mk), gmap)
    for w in wins[:6]:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        assert g.window_nodes().tobytes() == twin.window_nodes().tobytes() == nodes_ref(rows).tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_node_trend().tobytes() == twin.window_node_trend().tobytes()
        assert g.window_vanished().tobytes() == twin.window_vanished().tobytes()
        assert g.window_rank().tobytes() == twin.window_rank().tobytes()
        assert g.window_incidents().tobytes() == twin.window_incidents().tobytes()
        assert g.window_node_incident().tobytes() == twin.window_node_incident().tobytes()
        assert g.window_incident_tracks().tobytes() == twin.window_incident_tracks().tobytes()
        assert g.window_tracks_ended().tobytes() == twin.window_tracks_ended().tobytes()
        _check(g, rows, gmap, mk, mk)
    assert g.trend_entries().tobytes() == twin.trend_entries().tobytes()
    assert g.track_entries().tobytes() == twin.track_entries().tobytes()


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    mk = topo.n_nodes + 8
    for call in (g.window_groups, g.window_row_group, g.window_group_perm, g.window_groups_buffer):
        assert _rc(call) == engine.SG_ESTATE                           # the groups are off
    assert _rc(g.group_assign, [0], [0]) == engine.SG_ESTATE
    for bad in (dict(struct_size=12), dict(struct_size=20), dict(reserved=1), dict(reserved=(0, 1)), dict(max_groups=(1 << 30) + 1)):
        assert _rc(g.set_groups, **bad) == engine.SG_EINVAL
    _feed(g, wins[0]); g.flush_window()
    g.set_groups(max_groups=10)
    for call in (g.window_groups, g.window_row_group, g.window_group_perm, g.window_groups_buffer):
        assert _rc(call) == engine.SG_ESTATE                           # the read window was closed before they were on
    assert _rc(g.group_assign, [0], [10]) == engine.SG_EINVAL and _rc(g.group_assign, [mk], [0]) == engine.SG_EINVAL
    g.group_assign([0, 1, 2], [9, 9, NO])
    gmap = np.full(mk, NO, np.uint32); gmap[:2] = 9
    _feed(g, wins[1])
    _check(g, g.flush_window().copy(), gmap, 10, mk)
    g.set_groups(max_groups=10)                                       # again: the map starts over, the windows from here on
    assert _rc(g.window_groups) == engine.SG_ESTATE
    _feed(g, wins[2])
    _check(g, g.flush_window().copy(), np.full(mk, NO, np.uint32), 10, mk)
    g.set_groups(None)
    assert _rc(g.window_groups) == engine.SG_ESTATE and _rc(g.group_assign, [0], [0]) == engine.SG_ESTATE
    _feed(g, wins[3]); g.flush_window()
    assert _rc(g.window_groups) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_groups) == engine.SG_EINVAL
    assert _rc(g.window_groups) == engine.SG_ESTATE
