"""K20, the latency percentiles (sg_set_quantiles / sg_window_node_hist / sg_window_node_quantiles / their group and group-node twins
/ sg_window_quantiles_buffer): every histogram and every quantile byte for byte against tests/quantile_ref.py, computed from the
same engine's own window_hist(), rows, window_nodes(), window_groups(), window_group_perm() and window_group_nodes().  Shapes are
named after sg_quantiles.h's constants: C = 512 source positions a workgroup trip (K20_C), NR = 512 targets a range (K20_NR); the
engines have max_edges 16 384, so a scattered side has two slices (one per 8192 positions) and a sorted side eight (one per 2048)."""
import numpy as np
import pytest

from alaz_amd import engine, replay
from tests.gpu_scaffold import EXT, _d2h, _engine, _events, _feed, _hip, _pods_engine, _rc
from tests.helpers import G
from tests import quantile_ref as qr
from tests.traces import churn  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

C, NR = 512, 512
NO = engine.NO_GROUP
ALL = ("nodes", "groups", "group_nodes")
DEFAULT = (500, 990)


def _on(g, gmap=None, spaces=ALL, permille=DEFAULT):
    g.set_nodes(); g.set_groups()
    if gmap is not None:
        g.group_assign(np.arange(len(gmap)), gmap)
    g.set_group_nodes()
    g.set_quantiles(spaces, permille)


def _check(g, rows, permille=DEFAULT, spaces=ALL):
    """the last read window's tables in every space against the reference; returns them"""
    hist = g.window_hist()
    assert hist.shape == (len(rows), 16)
    out = {}
    if "nodes" in spaces:
        nodes = g.window_nodes()
        H, Q = g.window_node_hist(), g.window_node_quantiles()
        want = qr.fold_nodes(hist, rows, nodes)
        assert H.dtype == np.uint64 and H.shape == (len(nodes), 2, 16) and H.tobytes() == want.tobytes()
        assert Q.dtype == np.uint32 and Q.shape == (len(nodes), 2, len(permille))
        assert Q.tobytes() == qr.node_quantiles(want, nodes, permille).tobytes()
        assert np.array_equal(H[:, 0].sum(axis=1), nodes["out_count"]) and np.array_equal(H[:, 1].sum(axis=1), nodes["in_count"])
        out["nodes"] = (nodes, H, Q)
    if "groups" in spaces or "group_nodes" in spaces:
        ge, perm = g.window_groups(), g.window_group_perm()
    if "groups" in spaces:
        H, Q = g.window_group_hist(), g.window_group_quantiles()
        want = qr.fold_groups(hist, ge, perm)
        assert H.dtype == np.uint64 and H.shape == (len(ge), 16) and H.tobytes() == want.tobytes()
        assert Q.dtype == np.uint32 and Q.shape == (len(ge), len(permille))
        assert Q.tobytes() == qr.group_quantiles(want, ge, permille).tobytes()
        assert np.array_equal(H.sum(axis=1), ge["count"])
        out["groups"] = (ge, H, Q)
    if "group_nodes" in spaces:
        gn = g.window_group_nodes()
        H, Q = g.window_group_node_hist(), g.window_group_node_quantiles()
        want = qr.fold_group_nodes(hist, ge, perm, gn)
        assert H.shape == (len(gn), 2, 16) and H.tobytes() == want.tobytes()
        assert Q.shape == (len(gn), 2, len(permille)) and Q.tobytes() == qr.node_quantiles(want, gn, permille).tobytes()
        assert np.array_equal(H[:, 0].sum(axis=1), gn["out_count"]) and np.array_equal(H[:, 1].sum(axis=1), gn["in_count"])
        if "groups" in out:
            assert H.tobytes() == qr.fold_group_nodes_over_groups(out["groups"][1], ge, gn).tobytes()
        out["group_nodes"] = (gn, H, Q)
    return out


def _window(topo, g, src, dst, **kw):
    e = _events(topo, src, topo.pod_ips[np.asarray(dst, dtype=np.int64)], **kw)
    if len(e):
        g.ingest_bulk(e)
    return g.flush_window().copy()


def _durations(n, seed=0):
    """every bin, the octave boundaries on either side, bin 15 (>= 2^31 ns)"""
    edges = np.array([1, 1000, (1 << 17) - 1, 1 << 17] + [(1 << k) + d for k in range(18, 32) for d in (-1, 0, 1)] + [1 << 33, (1 << 40) + 12345],
                     dtype=np.uint64)
    return edges[np.random.default_rng(seed).integers(0, len(edges), n)]


# ---- 1. the sorted sides: runs at the trip and slice boundaries ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """4200 pods.  Workloads 0, 1, 2 = pods 2, 3, 4 (short runs in front); workload 5 = pod 10, the caller of the long run; workload
    6 = pods 100 .. 100 + 2 C: its callees.  A run of D rows is one node's out rows, one group edge (5 -> 6) and one workload's out
    rows at once, and the in side of workload 6"""
    topo, g, mk = _pods_engine(n_pods=4200, edge_histogram=True)
    gmap = np.full(mk, NO, np.uint32)
    gmap[[2, 3, 4, 10]] = [0, 1, 2, 5]; gmap[100:100 + 2 * C + 1] = 6
    _on(g, gmap)
    return topo, g, mk, gmap


@pytest.mark.parametrize("D", [1, 7, 8, 9, C - 1, C, C + 1, 2 * C + 1])
def test_sorted_runs_at_the_trip_and_slice_boundaries(wide, D):
    topo, g, mk, gmap = wide
    src = np.concatenate([[2, 2, 2], [3], [4, 4], np.full(D, 10), [50, 50, 51]])
    dst = np.concatenate([[60, 61, 62], [60], [60, 61], np.arange(D) + 100, [7, 8, 7]])
    rows = _window(topo, g, src, dst, dur=_durations(len(src), D))
    assert len(rows) == len(src)
    t = _check(g, rows)
    ge, H, _ = t["groups"]
    k = np.flatnonzero((ge["from_ref"] == G(5)) & (ge["to_ref"] == G(6)))
    assert len(k) == 1 and ge["edges"][k[0]] == D and H[k[0]].sum() == D
    gn, HW, _ = t["group_nodes"]
    assert HW[gn["ref"] == G(5)][0, 0].sum() == D and HW[gn["ref"] == G(6)][0, 1].sum() == D


# ---- 2. the scattered sides: entity counts at the range boundary, slices, hubs ---------------------------------------------------------
@pytest.mark.parametrize("n", [NR - 2, NR - 1, NR, NR + 1, NR + 2])
def test_entity_counts_around_a_range(wide, n):
    """pod 200 calls n - 1 ungrouped pods: n node rows and workload rows (NR - 1, NR, NR + 1 among them), n - 1 group edges"""
    topo, g, mk, gmap = wide
    rows = _window(topo, g, np.full(n - 1, 200), 1500 + np.arange(n - 1), dur=_durations(n - 1, n))
    t = _check(g, rows)
    assert len(t["nodes"][0]) == n == len(t["group_nodes"][0]) and len(t["groups"][0]) == n - 1


def test_hubs_slices_and_every_destination_type(wide):
    """9000 rows: more than one trip a slice on every side, several ranges.  One callee receives from every caller; pod 7 calls
    itself; destinations behind a Host label and raw outbound IPs; alive-only rows; a group edge inside workload 6"""
    topo, g, mk, gmap = wide
    rng = np.random.default_rng(11)
    src = np.concatenate([np.repeat(np.arange(40), 150), np.arange(2500), [7], np.arange(100, 300)])
    dst = np.concatenate([(np.arange(6000) * 7 + 300) % 4000, np.full(2500, 4100), [7], np.arange(101, 301)])
    pod = _events(topo, src, topo.pod_ips[dst], dur=_durations(len(src), 5), alive=rng.random(len(src)) < 0.05)
    ext = _events(topo, rng.integers(0, 4200, 300), EXT + rng.integers(0, 2, 300).astype(np.uint32), label=np.repeat([1, 2, 0], 100),
                  dur=_durations(300, 6))
    g.set_label_count(2)
    g.ingest_bulk(np.concatenate([pod, ext]))
    rows = g.flush_window().copy()
    assert len(rows) > 8 * C
    t = _check(g, rows)
    nodes, H, Q = t["nodes"]
    hub = np.flatnonzero(nodes["ref"] == nodes["ref"][np.argmax(nodes["in_edges"])])[0]
    assert nodes["in_edges"][hub] >= 2500 and H[hub, 1].sum() == nodes["in_count"][hub]
    assert {0, 1, 2} <= set((nodes["ref"] >> 30).tolist()) and (rows["count"] == 0).any()
    ge = t["groups"][0]
    assert ((ge["from_ref"] == G(6)) & (ge["to_ref"] == G(6))).any()
    # indexed reads against the full ones
    idx = rng.integers(0, len(nodes), 1500).astype(np.uint32)
    assert g.window_node_hist(idx).tobytes() == H[idx].tobytes() and g.window_node_quantiles(idx).tobytes() == Q[idx].tobytes()
    gi = rng.integers(0, len(ge), 37).astype(np.uint32)
    assert g.window_group_hist(gi).tobytes() == t["groups"][1][gi].tobytes() and g.window_group_quantiles(gi).tobytes() == t["groups"][2][gi].tobytes()
    gn, HW, QW = t["group_nodes"]
    wi = np.array([len(gn) - 1, 0, 0], np.uint32)
    assert g.window_group_node_hist(wi).tobytes() == HW[wi].tobytes() and g.window_group_node_quantiles(wi).tobytes() == QW[wi].tobytes()
    assert g.window_node_hist(np.zeros(0, np.uint32)).shape == (0, 2, 16)
    for call, cnt in ((g.window_node_hist, len(nodes)), (g.window_group_quantiles, len(ge)), (g.window_group_node_hist, len(gn))):
        assert _rc(call, np.array([cnt], np.uint32)) == engine.SG_EINVAL


def test_one_group_edge_folds_every_row():
    topo, g, mk = _pods_engine(n_pods=4200, edge_histogram=True)
    gmap = np.full(mk, NO, np.uint32); gmap[:4200] = 0
    _on(g, gmap)
    rows = _window(topo, g, np.arange(4000), (np.arange(4000) * 13 + 1) % 4200, dur=_durations(4000, 2))
    t = _check(g, rows)
    ge, H, Q = t["groups"]
    assert len(ge) == 1 and H[0].sum() == 4000 and len(t["group_nodes"][0]) == 1
    assert t["group_nodes"][1][0, 0].tobytes() == H[0].tobytes() == t["group_nodes"][1][0, 1].tobytes()


# ---- 3. values -----------------------------------------------------------------------------------------------------------------------
def test_values_caps_alive_only_and_small_windows(wide):
    topo, g, mk, gmap = wide
    none = np.zeros(0, np.int64)
    t = _check(g, _window(topo, g, none, none))                        # a window of no rows
    assert all(len(t[s][1]) == 0 for s in ALL)
    t = _check(g, _window(topo, g, [9], [11], dur=200_000))            # one row: bin 1 (2^17 <= d < 2^18), capped by max_ns = 200 us
    assert t["groups"][2].tolist() == [[200, 200]] and t["nodes"][2].tolist() == [[[200, 200], [0, 0]], [[0, 0], [200, 200]]]
    # 99 requests in bin 0 and one of 5 s: p50 = 131 us (the edge of bin 0), p99 = 131 us, p100 = the max
    g.set_quantiles(ALL, (500, 990, 1000, 1))
    dur = np.full(100, 1000, np.uint64); dur[37] = 5_000_000_000
    t = _check(g, _window(topo, g, np.full(100, 9), np.full(100, 11), dur=dur), (500, 990, 1000, 1))
    assert t["groups"][2].tolist() == [[131, 131, 5_000_000, 131]]
    # an alive-only window: every histogram and quantile zero; then alive-only rows beside requests
    t = _check(g, _window(topo, g, [9, 9, 12], [11, 12, 11], alive=[True, True, True]), (500, 990, 1000, 1))
    assert not t["nodes"][1].any() and not t["nodes"][2].any() and not t["groups"][2].any() and len(t["groups"][0]) == 3
    t = _check(g, _window(topo, g, [9, 9, 12], [11, 12, 11], alive=[False, True, False], dur=[1 << 20, 0, (1 << 31) + 5]), (500, 990, 1000, 1))
    g.set_quantiles(ALL)


@pytest.mark.parametrize("permille", [(1,), (1000,), (1, 250, 500, 750, 900, 990, 999, 1000)], ids=["q1", "q1000", "eight"])
def test_one_and_eight_quantiles(wide, permille):
    topo, g, mk, gmap = wide
    g.set_quantiles(ALL, permille)
    rng = np.random.default_rng(4)
    rows = _window(topo, g, rng.integers(0, 30, 3000), rng.integers(0, 4200, 3000), dur=_durations(3000, 9))
    _check(g, rows, permille)
    g.set_quantiles(ALL)


# ---- 4. links to what is already pinned --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_nothing_grouped_and_every_pass_a_variant(churn, variant):
    """under a map that groups nothing a group edge is a row: its histogram is the row's, its quantiles at {500, 990} the row's
    p50_us / p99_us, and the workload space is the node space; one shape over k1_variant 0, 1 and 2"""
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=variant, max_edges=1 << 14, edge_histogram=True)
    _on(g)
    for w in wins[:2]:
        _feed(g, w)
        rows = g.flush_window().copy()
        t = _check(g, rows)
        ge, H, Q = t["groups"]
        perm = g.window_group_perm()
        assert len(ge) == len(rows) and H.tobytes() == g.window_hist()[perm].astype(np.uint64).tobytes()
        assert np.array_equal(Q[:, 0], rows["p50_us"][perm]) and np.array_equal(Q[:, 1], rows["p99_us"][perm])
        assert t["group_nodes"][1].tobytes() == t["nodes"][1].tobytes() and t["group_nodes"][2].tobytes() == t["nodes"][2].tobytes()


def test_a_twin_without_the_stage_is_unchanged(churn):
    topo, labels, wins = churn
    g, twin = (_engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True) for _ in range(2))
    gmap = np.full(topo.n_nodes + 8, NO, np.uint32); gmap[:topo.n_pods] = np.arange(topo.n_pods) // 7
    _on(g, gmap)
    twin.set_nodes(); twin.set_groups(); twin.group_assign(np.arange(len(gmap)), gmap); twin.set_group_nodes()
    for w in wins[:3]:
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        _check(g, rows)
        for call in ("window_nodes", "window_groups", "window_group_nodes", "window_group_perm", "window_hist"):
            assert getattr(g, call)().tobytes() == getattr(twin, call)().tobytes(), call


# ---- 5. close paths, windows in flight, lifecycle ----------------------------------------------------------------------------------------
def test_every_close_path(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    gmap = np.full(topo.n_nodes + 8, NO, np.uint32); gmap[:topo.n_pods] = np.arange(topo.n_pods) // 7
    _on(g, gmap)
    for i, w in enumerate(wins[:7]):
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_node_hist, g.window_group_quantiles, g.window_group_node_hist, g.set_quantiles):
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            rows = g.flush_end().copy()
        elif i == 1:
            rows = g.flush_window_view().copy()
        elif i == 2:
            g.flush_begin(); rows = g.flush_end_view().copy()
        elif i == 3:
            g.flush_window_top(3); rows = None
        elif i == 4:
            g.window_run(); rows = g.window_read().copy()
        elif i == 5:
            g.window_close(); g.window_features()
            for l in range(2):
                g.window_layer(l)
            g.window_score(); rows = g.window_read().copy(); g.window_reset()
        else:
            rows = g.flush_window().copy()
        if rows is None:                                              # the _top flush returns a selection: the full rows are a twin's
            twin = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
            _feed(twin, w)
            rows = twin.flush_window().copy()
        _check(g, rows)


def test_window_run_three_in_flight_through_the_device_buffers(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True, windows_in_flight=3)
    one = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    gmap = np.full(topo.n_nodes + 8, NO, np.uint32); gmap[:topo.n_pods] = np.arange(topo.n_pods) // 5
    permille = (500, 990, 999)
    for x in (g, one):
        _on(x, gmap, permille=permille)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(wins[:6]):
        _feed(one, w)
        t = _check(one, one.flush_window().copy(), permille)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((t, [g.window_quantiles_buffer(s) for s in ALL]))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for t, bufs in pending:
                for s, (hp, qp) in zip(ALL, bufs):
                    _, H, Q = t[s]
                    sides = H.size // (len(H) * 16) if len(H) else 1
                    assert _d2h(hip, hp, H.size, np.uint64).tobytes() == H.tobytes()
                    q = _d2h(hip, qp, len(H) * sides * engine.Q_MAX, np.uint32).reshape(len(H), sides, engine.Q_MAX)
                    assert q[:, :, :3].tobytes() == Q.reshape(len(H), sides, 3).tobytes()
                sizes.append(len(t["nodes"][0]))
            pending = []
    assert len(sizes) == 6 and len(set(sizes)) > 1


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    plain = _engine(topo, labels, variant=2, max_edges=1 << 14)
    plain.set_nodes()
    assert _rc(plain.set_quantiles, "nodes") == engine.SG_ESTATE      # an engine without the histogram
    g = _engine(topo, labels, variant=2, max_edges=1 << 14, edge_histogram=True)
    for sp in ALL:
        assert _rc(g.set_quantiles, sp) == engine.SG_ESTATE           # a space without its base stage
    g.set_nodes()
    g.set_quantiles("nodes")
    assert _rc(g.set_quantiles, "groups") == engine.SG_ESTATE         # (a refused call leaves the setting as it was)
    assert _rc(g.window_node_hist) == engine.SG_ESTATE                # no window closed with it on yet
    assert _rc(g.window_group_hist) == engine.SG_ESTATE and _rc(g.window_quantiles_buffer, "group_nodes") == engine.SG_ESTATE
    for bad in ((0,), (1001,), (500, 0)):
        assert _rc(g.set_quantiles, "nodes", bad) == engine.SG_EINVAL
    assert _rc(g.set_quantiles, "nodes", tuple(range(1, 10))) == engine.SG_EINVAL    # n_q = 9
    assert _rc(g.set_quantiles, 8) == engine.SG_EINVAL and _rc(g.window_quantiles_buffer, 3) == engine.SG_EINVAL
    _feed(g, wins[0])
    rows = g.flush_window().copy()
    _check(g, rows, spaces=("nodes",))                                # the failed calls left the stage as it was
    g.set_groups(); g.set_group_nodes()
    g.set_quantiles(ALL, ())                                          # n_q = 0: {500, 990}
    assert _rc(g.window_node_hist) == engine.SG_ESTATE                # the window was closed before this setting
    _feed(g, wins[1])
    _check(g, g.flush_window().copy())
    g.set_group_nodes(False)                                          # a base stage switched off underneath: its space goes, the others stay
    assert _rc(g.window_group_node_hist) == engine.SG_ESTATE and len(g.window_group_hist()) and len(g.window_node_hist())
    g.set_nodes(False)
    assert _rc(g.window_node_quantiles) == engine.SG_ESTATE and len(g.window_group_quantiles())
    g.set_groups()                                                    # any sg_set_groups frees what is behind it
    assert _rc(g.window_group_hist) == engine.SG_ESTATE
    g.set_quantiles("groups")
    _feed(g, wins[2])
    _check(g, g.flush_window().copy(), spaces=("groups",))
    g.set_quantiles(None)
    assert _rc(g.window_group_hist) == engine.SG_ESTATE
    _feed(g, wins[3])
    g.flush_window()
    g.set_quantiles("groups")
    assert _rc(g.window_group_hist) == engine.SG_ESTATE               # a window closed while the stage was off
