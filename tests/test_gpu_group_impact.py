"""K22, the workload impact (sg_set_group_impact / sg_window_group_impact / sg_window_group_node_hops / sg_window_group_impact_mask /
sg_window_group_impact_buffer): the impact rows, the hops and the mask rows of every window against the pure-Python reference
tests/impact_ref.py run on the device's own window_groups(), window_group_nodes(), window_group_incidents() and
window_group_node_incident() of that window — byte for byte, every value is an integer.

The constructed windows run under the map that groups nothing: each pod is its own workload row, and pod -> pod events make the
group edges.  Which group edges are red is steered through K15: every window is sent twice, first with one latency on every edge
(the baseline's warm-up of one window), then with the edges that are to be red two hundred times slower; the incidents are keyed by
lat_dev.  tests/test_group_impact_host.py holds the same shapes to the references on the CPU."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import _d2h, _engine, _events, _feed, _grouped, _hip, _pods_engine, _rc
from tests.group_ref import group_ref
from tests.helpers import G
from tests.impact_ref import impact_ref
from tests.incident_ref import quantile_threshold
from tests.traces import churn  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

NO = engine.NO_INCIDENT
NOG = engine.NO_GROUP
NOH = engine.NO_HOPS
INF = float("inf")
FAST, SLOW = 1_000_000, 200_000_000
(EXPOSED, DIRECT, FAR, ENTRIES, ENTRY_COUNT, ENTRY_ERR, INTO_COUNT, INTO_ERR) = range(8)


def _check(g, mi, mh, ge=None, gn=None, incs=None, inc=None, got=None):
    """the last read window's impact rows, hops and mask rows (or `got`) against the reference over the device's own group edges,
    workload rows, incidents and incident per workload row"""
    ge = g.window_groups() if ge is None else ge
    gn = g.window_group_nodes() if gn is None else gn
    n_inc = len(g.window_group_incidents()) if incs is None else incs
    inc = g.window_group_node_incident() if inc is None else inc
    want = impact_ref(ge, gn, n_inc, inc, mi, mh)
    got = (g.window_group_impact(), g.window_group_node_hops(), g.window_group_impact_mask()) if got is None else got
    for name, a, b in zip(("impact", "hops", "mask"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (name, mi, mh)
    return got[0], got[1], got[2], gn, inc


def _window(topo, g, src, dst, red, mi=256, mh=8, daddr=None, alive=None, rows_out=None):
    """the (src pod, dst pod) pairs as one window, the pairs at `red` (a boolean mask) as its red group edges; checked.  rows_out: a
    list that gets the window's edge rows"""
    src, red = np.asarray(src, dtype=np.int64), np.asarray(red, bool)
    daddr = topo.pod_ips[np.asarray(dst, dtype=np.int64)] if daddr is None else daddr
    g.set_group_trend(shift=1, warmup=1, ttl=8)                         # an empty baseline
    g.set_group_incidents(by="lat_dev", min_value=3.0)
    g.set_group_impact(mi, mh)
    for dur in (np.full(len(src), FAST), np.where(red, SLOW, FAST)):
        g.ingest_bulk(_events(topo, src, daddr, dur=dur, alive=alive))
        rows = g.flush_window().copy()
    if rows_out is not None:
        rows_out.append(rows)
    assert len(g.window_group_incidents()) > 0
    return _check(g, mi, mh)


@pytest.fixture(scope="module")
def pods():
    """4200 pods under the map that groups nothing, K16 on"""
    topo, g, mk = _pods_engine(n_pods=4200)
    g.set_groups(); g.set_group_nodes()
    return topo, g, mk


# ---- 1 - 3. chains, a diamond, a cycle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("down", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("mh", [11, 12, 4])
def test_a_chain_of_12_rows_into_one_red_edge(pods, down, mh):
    """c0 -> c1 -> ... -> c11 -> c12 with the last edge red: rows c0 .. c10 are 11, 10, ... 1 call edges from the incident.  The ids
    ascend towards the incident or descend: a search that moved a bit more than one hop per launch fails one of the two"""
    topo, g, mk = pods
    c = (112 - np.arange(13)) if down else (100 + np.arange(13))
    rows, hops, mask, gn, inc = _window(topo, g, c[:-1], c[1:], np.arange(12) == 11, mh=mh)
    at = {int(r): v for v, r in enumerate(gn["ref"])}
    d = [11 - k for k in range(11)] + [0, 0]
    assert [int(hops[at[int(x)]]) for x in c] == [x if x <= mh else NOH for x in d]
    assert len(rows) == 1 and rows[0, EXPOSED] == min(11, mh) and rows[0, DIRECT] == 1
    assert int(rows[0, FAR]) == min(11, mh) << 32 | at[int(c[11 - min(11, mh)])]
    assert rows[0, ENTRIES] == (1 if mh >= 11 else 0)


def test_a_diamond_and_a_cycle(pods):
    topo, g, mk = pods
    # 50 -> 59 and 50 -> 51 -> 52 -> 59, 59 -> 60 red: paths of 1 and 3 hops to the same member, the shorter wins
    src, dst = [50, 50, 51, 52, 59], [59, 51, 52, 59, 60]
    rows, hops, mask, gn, inc = _window(topo, g, src, dst, np.arange(5) == 4)
    assert hops.tolist() == [1, 2, 1, 0, 0] and rows[0].tolist()[:2] == [3, 2] and int(rows[0, FAR]) == 2 << 32 | 1
    # 70 -> 71 -> 72 -> 70 through the member 70 (70 -> 75 red): it ends, 72 is 1 away and 71 is 2
    rows, hops, mask, gn, inc = _window(topo, g, [70, 71, 72, 70], [71, 72, 70, 75], np.arange(4) == 3)
    assert hops.tolist() == [0, 2, 1, 0] and rows[0, EXPOSED] == 2 and rows[0, ENTRIES] == 0


# ---- 4. word boundaries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mi", [(65, 1), (65, 64), (65, 65), (65, 100), (129, 64), (129, 65), (129, 100), (129, 256)])
def test_incidents_across_the_mask_words(pods, n, mi):
    """n single-edge incidents 2i -> 2i + 1, each with its own caller 1000 + i, and pod 999 calling a member of every incident: with
    129 covered incidents its mask has bits 63, 64 and 128 set; the bits of uncovered incidents are 0"""
    topo, g, mk = pods
    i = np.arange(n)
    src = np.concatenate([2 * i, 1000 + i, np.full(n, 999)])
    dst = np.concatenate([2 * i + 1, 2 * i, 2 * i])
    rows, hops, mask, gn, inc = _window(topo, g, src, dst, np.arange(3 * n) < n, mi=mi)
    cov = min(n, mi)
    assert len(rows) == cov and mask.shape == (len(gn), (mi + 63) // 64)
    at = {int(r): v for v, r in enumerate(gn["ref"])}
    bits = sum(int(mask[at[999], w]) << (64 * w) for w in range(mask.shape[1]))
    assert bits == (1 << cov) - 1
    assert (rows[:, EXPOSED] == 2).all() and (rows[:, ENTRIES] == 2).all()
    assert [int(hops[at[1000 + k]]) for k in range(n)] == [1 if k < mi else NOH for k in range(n)]


# ---- 5, 6. the folds ---------------------------------------------------------------------------------------------------------------------
def test_more_incidents_through_one_workgroup_than_its_table_has_slots(pods):
    """600 incidents 1000 + 2i -> 1001 + 2i; their callers are pods 0 .. 255, the first 256 workload rows — one workgroup's span of
    k22_pull — and pod c calls incidents c, c + 256 and c + 512: that workgroup folds 600 distinct incidents into a table of 512"""
    topo, g, mk = pods
    i = np.arange(600)
    src = np.concatenate([1000 + 2 * i, i % 256])
    dst = np.concatenate([1001 + 2 * i, 1000 + 2 * i])
    rows, hops, mask, gn, inc = _window(topo, g, src, dst, np.arange(1200) < 600, mi=1024)
    assert len(rows) == 600 and (rows[:, EXPOSED] == 1).all() and (rows[:, DIRECT] == 1).all() and (hops[:256] == 1).all()
    assert (rows[:, INTO_COUNT] == 1).all() and (rows[:, ENTRIES] == 1).all()


def test_one_incident_with_3000_direct_callers(pods):
    topo, g, mk = pods
    src = np.concatenate([[10], np.arange(1000, 4000)])
    dst = np.concatenate([[11], np.full(3000, 10)])
    rows, hops, mask, gn, inc = _window(topo, g, src, dst, np.arange(3001) == 0)
    assert rows[0].tolist()[:2] == [3000, 3000] and int(rows[0, FAR]) == 1 << 32 | 2 and rows[0, ENTRIES] == 3000
    assert rows[0, INTO_COUNT] == 3000 and rows[0, ENTRY_COUNT] == 3000


# ---- 7. edge kinds -----------------------------------------------------------------------------------------------------------------------
def test_alive_only_and_within_workload_edges_expose_nobody():
    """workload 0 = pods 20, 21; 20 -> 30 red.  21 -> 20 is traffic inside the workload and 40 -> 20 an alive-only edge: neither
    exposes anybody.  The frontend 41 calls the workload and itself: exposed, and still an entry"""
    topo, g, mk = _pods_engine(n_pods=64)
    g.set_groups(); g.group_assign([20, 21], [0, 0]); g.set_group_nodes()
    src, dst = np.array([20, 21, 40, 41, 41]), np.array([30, 20, 20, 41, 20])
    rows, hops, mask, gn, inc = _window(topo, g, src, dst, np.arange(5) == 0, alive=np.arange(5) == 2)
    at = {int(r): v for v, r in enumerate(gn["ref"])}
    assert hops[at[40]] == NOH and hops[at[41]] == 1 and hops[at[G(0)]] == 0 and hops[at[30]] == 0
    assert rows[0, EXPOSED] == 1 and rows[0, ENTRIES] == 1 and rows[0, ENTRY_COUNT] == int(gn["out_count"][at[41]]) == 2
    assert rows[0, INTO_COUNT] == 1


# ---- 8. row counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_row_counts_around_a_workgroups_span(pods, n):
    """a chain of n workload rows into a red last edge, cut at 64 hops"""
    topo, g, mk = pods
    ids = 50 + np.arange(n)
    rows, hops, mask, gn, inc = _window(topo, g, ids[:-1], ids[1:], np.arange(n - 1) == n - 2, mh=64)
    assert len(gn) == n and rows[0, EXPOSED] == 64 and int(rows[0, FAR]) == 64 << 32 | (n - 2 - 64)
    assert hops.tolist() == [NOH] * (n - 66) + list(range(64, 0, -1)) + [0, 0]


# ---- 9. services bound to the workload behind them ---------------------------------------------------------------------------------------
def test_services_bound_to_their_workloads_join_the_chain():
    """frontend -> checkout-svc, checkout -> payments-svc, payments -> db-svc, the last edge red.  With the three Service ids assigned
    to the workloads behind them the window is the chain frontend -> checkout -> payments -> db: hops 2, 1, 0, 0, two exposed rows
    and one entry, frontend.  On the twin without those assignments the incident is payments and db-svc, and nobody calls either:
    checkout calls payments-svc, another row.  (The contract gives 0 exposed rows there; every chain ends after one hop.)"""
    out = []
    for bound in (True, False):
        topo, g, mk = _pods_engine(n_pods=8)
        P = topo.n_pods
        g.set_groups(); g.group_assign([0, 1, 2, 3], [0, 1, 2, 3]); g.set_group_nodes()
        gmap = np.full(mk, NOG, np.uint32); gmap[:4] = [0, 1, 2, 3]
        if bound:
            g.group_assign([P, P + 1, P + 2], [1, 2, 3]); gmap[P:P + 3] = [1, 2, 3]
        edge_rows = []
        rows, hops, mask, gn, inc = _window(topo, g, [0, 1, 2], None, np.arange(3) == 2, daddr=topo.svc_ips[:3], rows_out=edge_rows)
        want, _, _ = group_ref(edge_rows[0], gmap, mk, mk, 16)
        ge = g.window_groups()
        for f in ge.dtype.names:
            assert ge[f].tobytes() == want[f].tobytes(), f
        out.append((rows, hops, gn))
    (rows, hops, gn), (trows, thops, tgn) = out
    assert gn["ref"].tolist() == [G(0), G(1), G(2), G(3)] and hops.tolist() == [2, 1, 0, 0]
    assert rows[0, EXPOSED] == 2 and rows[0, ENTRIES] == 1 and int(rows[0, FAR]) == 2 << 32 | 0
    assert rows[0, ENTRY_COUNT] == int(gn["out_count"][0])
    assert len(tgn) == 6 and trows[0, EXPOSED] == 0 and int((thops != NOH).sum()) == 2


# ---- 10. the churn -----------------------------------------------------------------------------------------------------------------------
def test_churn_against_a_twin_without_it(churn):
    """K15 - K19 and K22 on against a twin without K22: every other output is byte-identical, the twin's impact reads are SG_ESTATE,
    and every window is held to the reference, at two thresholds (the 0.9 and the 0.99 quantile of the window before)"""
    topo, labels, wins = churn
    (g, _, mk), (twin, _, _) = _grouped(topo, labels, "blocks"), _grouped(topo, labels, "blocks")
    for x in (g, twin):
        x.set_group_trend(shift=3, warmup=2, ttl=3); x.set_group_nodes(); x.set_group_node_trend(shift=3, warmup=2, ttl=2); x.set_group_rank(iters=3)
    thr, exposed, far = 0.0, 0, 0
    for i, w in enumerate(wins[:8]):
        for x in (g, twin):
            x.set_group_incidents(by="score", min_value=thr); x.set_group_tracks()
        g.set_group_impact(64, 8)
        _feed(g, w); _feed(twin, w)
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        ge = g.window_groups()
        assert ge.tobytes() == twin.window_groups().tobytes()
        assert g.window_group_trend().tobytes() == twin.window_group_trend().tobytes()
        assert g.window_group_nodes().tobytes() == twin.window_group_nodes().tobytes()
        assert g.window_group_node_trend().tobytes() == twin.window_group_node_trend().tobytes()
        assert g.window_group_rank().tobytes() == twin.window_group_rank().tobytes()
        assert g.window_group_incidents().tobytes() == twin.window_group_incidents().tobytes()
        assert g.window_group_node_incident().tobytes() == twin.window_group_node_incident().tobytes()
        assert g.window_group_incident_tracks().tobytes() == twin.window_group_incident_tracks().tobytes()
        rows = _check(g, 64, 8, ge=ge)[0]
        exposed += int(rows[:, EXPOSED].sum()); far = max(far, int(rows[:, FAR].max() >> np.uint64(32)) if len(rows) else 0)
        thr = quantile_threshold(ge["score_max"], 0.9 if i % 2 == 0 else 0.99)
    assert exposed > 0 and 2 <= far < 0xFFFFFFFF
    for call in (twin.window_group_impact, twin.window_group_node_hops, twin.window_group_impact_mask, twin.window_group_impact_buffer):
        assert _rc(call) == engine.SG_ESTATE


# ---- 11. close paths ---------------------------------------------------------------------------------------------------------------------
def test_every_close_path(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    g.set_group_nodes()
    thr = 0.0
    for i, w in enumerate(wins[:7]):
        g.set_group_incidents(by="score", min_value=thr); g.set_group_impact(100, 6)
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_group_impact, g.window_group_node_hops, g.window_group_impact_mask, g.set_group_impact):
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            assert _rc(g.set_group_impact, None) == engine.SG_ESTATE
            g.flush_end()
        elif i == 1:
            g.flush_window_view()
        elif i == 2:
            g.flush_begin(); g.flush_end_view()
        elif i == 3:
            g.flush_window_top(3)
        elif i == 4:
            g.window_run(); g.window_read()
        elif i == 5:
            g.window_close(); g.window_features()
            for l in range(2):
                g.window_layer(l)
            g.window_score(); g.window_read(); g.window_reset()
        else:
            g.flush_window()
        ge = g.window_groups()
        rows = _check(g, 100, 6, ge=ge)[0]
        assert i == 0 or len(rows) > 0
        thr = quantile_threshold(ge["score_max"], 0.9)


def test_window_run_with_three_windows_in_flight(churn):
    """each window's impact rows, hops and mask rows are read from its own slot's buffers after the whole round was enqueued, and held
    to the reference over a one-call engine's group edges and workload rows and the slot's own incidents"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=3), _engine(topo, labels)
    for x in (g, one):
        x.set_groups(); x.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 5); x.set_group_nodes()
    mi, mh, W = 70, 5, 2
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    thr, pending, seen = None, [], []
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        one.flush_window()
        ge, gn = one.window_groups(), one.window_group_nodes()
        if thr is None:                                               # (nothing is in flight yet: the switches may allocate)
            thr = quantile_threshold(ge["score_max"], 0.9)
            g.set_group_incidents(by="score", min_value=thr); g.set_group_impact(mi, mh)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((ge, gn, g.window_group_incidents_buffer(), g.window_group_impact_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            assert len({p[3] for p in pending}) == 3                   # three slots, three sets of buffers
            for ge, gn, (ip, cp, np_), (rp, rc, hp, mp) in pending:
                n_inc = int(_d2h(hip, cp, 1, np.uint64)[0])
                cov = int(_d2h(hip, rc, 1, np.uint64)[0])
                assert cov == min(n_inc, mi)
                got = (_d2h(hip, rp, cov * 8, np.dtype("<u8")).reshape(cov, 8), _d2h(hip, hp, len(gn), np.dtype("<u4")),
                       _d2h(hip, mp, len(gn) * W, np.dtype("<u8")).reshape(len(gn), W))
                _check(g, mi, mh, ge=ge, gn=gn, incs=n_inc, inc=_d2h(hip, np_, len(gn), np.uint32), got=got)
                seen.append(int(got[0][:, EXPOSED].sum()) if cov else 0)
            pending = []
    assert len(seen) == 9 and max(seen) > 0


# ---- 12. lifecycle -----------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    reads = (g.window_group_impact, g.window_group_node_hops, g.window_group_impact_mask, g.window_group_impact_buffer)

    def off():
        for call in reads:
            assert _rc(call) == engine.SG_ESTATE

    def err(call, *a):
        with pytest.raises(engine.ServiceGraphError) as ei:
            call(*a)
        return ei.value.rc, str(ei.value).split(": ", 1)[1]

    assert err(g.set_group_impact) == (engine.SG_ESTATE, "sg_set_group_impact: the workload incidents are off (sg_set_group_incidents)")
    assert _rc(g.set_group_impact, None) == engine.SG_ESTATE
    g.set_groups(); g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7); g.set_group_nodes()
    assert _rc(g.set_group_impact) == engine.SG_ESTATE
    off()
    g.set_group_incidents(min_value=0.5)
    assert err(g.window_group_impact) == (engine.SG_ESTATE, "sg_window_group_impact: the workload impact is off (sg_set_group_impact)")
    for bad in ((0, 8), (8, 0), (1025, 8), (8, 65), (0xFFFFFFFF, 1)):
        assert err(g.set_group_impact, *bad) == (engine.SG_EINVAL, "sg_set_group_impact: bad parameters")
    _feed(g, wins[0]); g.flush_window()
    thr = quantile_threshold(g.window_groups()["score_max"], 0.9)     # (several incidents a window)
    g.set_group_incidents(min_value=thr); g.set_group_impact()
    assert err(g.window_group_node_hops) == (engine.SG_ESTATE, "sg_window_group_node_hops: the last read window was closed while the workload impact was off")
    off()
    _feed(g, wins[1]); g.flush_window()
    rows, hops, mask, gn, inc = _check(g, 256, 8)
    assert mask.shape[1] == 4
    # the index form: repeats, empty, out of range, a cap below the count
    n = len(gn)
    rep = np.array([5, 5, 0, n - 1, 5], np.uint32)
    assert g.window_group_node_hops(rep).tolist() == hops[rep].tolist()
    assert len(g.window_group_node_hops(np.zeros(0, np.uint32))) == 0
    assert err(g.window_group_node_hops, np.array([0, n], np.uint32)) == (engine.SG_EINVAL, "sg_window_group_node_hops: a node index beyond the window's workload rows")
    out = np.full(5, 0xFFFFFFFF - 1, np.uint32)
    cnt = C.c_size_t(0)
    assert g._l.sg_window_group_node_hops(g._h, rep.ctypes.data, 5, out.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == 5 and out[:3].tolist() == hops[rep[:3]].tolist() and out[3:].tolist() == [0xFFFFFFFF - 1] * 2
    few = np.zeros((1, 8), np.dtype("<u8"))
    assert g._l.sg_window_group_impact(g._h, few.ctypes.data, 1, C.byref(cnt)) == 0
    assert cnt.value == len(rows) >= 1 and few[0].tolist() == rows[0].tolist()
    # on again with other parameters: the windows from here on
    g.set_group_impact(3, 2)
    off()
    _feed(g, wins[2]); g.flush_window()
    assert _check(g, 3, 2)[2].shape[1] == 1
    g.set_group_impact(None)
    off()
    g.set_group_impact(65, 64)
    _feed(g, wins[3]); g.flush_window()
    assert _check(g, 65, 64)[2].shape[1] == 2
    # any sg_set_group_incidents call switches it off, on or off
    g.set_group_incidents(min_value=thr)
    off()
    _feed(g, wins[4]); g.flush_window()
    off()
    assert len(g.window_group_incidents()) > 0
    g.set_group_impact(8, 8)
    g.set_group_incidents(None)
    off()
    assert _rc(g.set_group_impact) == engine.SG_ESTATE
    g.set_group_incidents(min_value=thr); g.set_group_impact(8, 8)
    g.set_group_nodes(False)                                          # the workload rows off take the incidents and the stage with them
    off()
    g.set_group_nodes(); g.set_group_incidents(min_value=thr); g.set_group_impact(8, 8)
    _feed(g, wins[5]); g.flush_window()
    _check(g, 8, 8)
    # what does not touch it: the map, K17, K19
    g.group_assign([0, 1], [5, NOG]); g.set_group_rank(iters=2); g.set_group_tracks()
    _feed(g, wins[6]); g.flush_window()
    _check(g, 8, 8)
    g.set_groups()                                                    # any sg_set_groups call frees it
    off()
