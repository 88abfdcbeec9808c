"""K18, the workload incidents (sg_set_group_incidents / sg_window_group_incidents / sg_window_group_node_incident /
sg_window_group_incidents_buffer): the incident rows and the incident per workload row of every window against the pure-Python
reference tests/group_incident_ref.py run on the device's own window_groups(), window_group_nodes(), window_group_trend() and
window_group_rank() of that window — byte for byte, every field is an integer or a max of float bits; under the map that groups
nothing against K12's incidents of the same engine; an engine with it against a twin without it; constructed windows whose
components are known (long chains hooked in both directions, every CAS on one root, more incidents through one workgroup than its
LDS table has slots); every close path and sg_window_run with three windows in flight; the lifecycle; and a rollout through which
the workload incident keeps its names while K12's pods change."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _d2h, _engine, _events, _feed, _grouped, _hip, _pairs, _pods_engine, _rc, _send
from tests.group_incident_ref import group_incident_ref, group_values
from tests.helpers import CLOCK, G, HostShim
from tests.incident_ref import quantile_threshold
from tests.traces import churn  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

NO = engine.NO_INCIDENT
NOG = engine.NO_GROUP
INF = float("inf")
EXT = 0x5DB8D800                                                      # addresses outside the cluster
TREND = dict(shift=3, warmup=2, ttl=4)
BYS = ("score", "lat_dev", "err_dev")


def _check(g, by="score", thr=0.0, ranked=False, ge=None, gn=None, trend=None, rank=None, got=None, ginc=None):
    """the last read window's workload incidents (or `got`, `ginc`) against the reference over the device's own group edges,
    workload rows and — for a trend key / with K17 on — group trend rows and workload rank rows"""
    ge = g.window_groups() if ge is None else ge
    gn = g.window_group_nodes() if gn is None else gn
    if by != "score" and trend is None:
        trend = g.window_group_trend()
    if ranked and rank is None:
        rank = g.window_group_rank()
    want, winc = group_incident_ref(ge, gn, by, thr, trend=trend, rank=rank)
    got = g.window_group_incidents() if got is None else got
    ginc = g.window_group_node_incident() if ginc is None else ginc
    assert len(got) == len(want), (len(got), len(want), by, thr)
    assert got.tobytes() == want.tobytes(), (by, thr)
    assert ginc.tobytes() == winc.tobytes()
    assert (got["culprit_node"] == NO).all() == (rank is None or len(got) == 0)
    return got


# ---- 1. the churn ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
def test_churn_under_three_maps(churn, kind):
    """one engine per threshold — -inf, +inf and the 0.5 / 0.9 / 0.99 quantiles of the window's own values, taken from a twin that
    closes the window first (every engine sees every window once: the baselines agree); the key and K17 change from window to
    window.  "none" with K9, K11 and K12 on too: where the key is the score the workload incidents are K12's of the same engine"""
    topo, labels, wins = churn
    specs = [-INF, INF, 0.5, 0.9, 0.99]
    twin = _grouped(topo, labels, kind)[0]
    gs = [_grouped(topo, labels, kind)[0] for _ in specs]
    for x in [twin] + gs:
        x.set_group_trend(**TREND); x.set_group_nodes()
        if kind == "none":
            x.set_nodes()
    counts, sizes, same = set(), set(), 0
    for i, w in enumerate(wins):
        by, ranked = BYS[i % 3], (i // 3) % 2 == 1
        _feed(twin, w)
        twin.flush_window()
        val = group_values(twin.window_groups(), by, twin.window_group_trend())
        for g, q in zip(gs, specs):
            thr = q if abs(q) == INF else quantile_threshold(val, q)
            g.set_group_rank(iters=3) if ranked else g.set_group_rank(None)
            g.set_group_incidents(by=by, min_value=thr)
            if kind == "none":
                g.set_rank(iters=3) if ranked else g.set_rank(None)
                g.set_incidents(by="score", min_value=thr)
            _feed(g, w)
            n_rows = len(g.flush_window())
            ge = g.window_groups()
            got = _check(g, by, thr, ranked, ge=ge)
            counts.add(len(got))
            sizes.add(int(got["nodes"].max()) if len(got) else 0)
            if q == INF:
                assert len(got) == 0
            if q == -INF:
                assert int(got["edges"].sum()) == int((~np.isnan(val)).sum())
            if kind == "none" and by == "score":
                assert len(ge) == n_rows and got.tobytes() == g.window_incidents().tobytes()
                assert g.window_group_node_incident().tobytes() == g.window_node_incident().tobytes()
                same += len(got)
    # ("one": every pod is in workload 0 and every row has a pod at one end, so every red group edge touches row 0: one incident at most)
    assert 0 in counts and 1 in counts and (max(counts) == 1 if kind == "one" else max(counts) > 3) and max(sizes) >= 3, (counts, sizes)
    assert same > 0 or kind != "none"


def test_a_twin_without_it_is_unchanged(churn):
    """rows, group edges, K15's output, workload rows, their trend and K17's rows of an engine with the stage against a twin
    without it; the twin's reads are SG_ESTATE"""
    topo, labels, wins = churn
    (g, _, mk), (twin, _, _) = _grouped(topo, labels, "blocks"), _grouped(topo, labels, "blocks")
    for x in (g, twin):
        x.set_group_trend(shift=3, warmup=2, ttl=3); x.set_group_vanished(silent_windows=1, min_seen=1)
        x.set_group_nodes(); x.set_group_node_trend(shift=3, warmup=2, ttl=2); x.set_group_rank(iters=3)
    thr = 0.0
    for i, w in enumerate(wins[:8]):
        by = BYS[i % 3]
        g.set_group_incidents(by=by, min_value=thr)
        _feed(g, w); _feed(twin, w)
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        ge, tr = g.window_groups(), g.window_group_trend()
        assert ge.tobytes() == twin.window_groups().tobytes()
        assert g.window_row_group().tobytes() == twin.window_row_group().tobytes()
        assert tr.tobytes() == twin.window_group_trend().tobytes()
        assert g.window_group_vanished().tobytes() == twin.window_group_vanished().tobytes()
        assert g.window_group_nodes().tobytes() == twin.window_group_nodes().tobytes()
        assert g.window_group_node_trend().tobytes() == twin.window_group_node_trend().tobytes()
        assert g.window_group_rank().tobytes() == twin.window_group_rank().tobytes()
        _check(g, by, thr, True, ge=ge, trend=tr)
        thr = quantile_threshold(group_values(ge, BYS[(i + 1) % 3], tr), 0.9)
    assert g.group_trend_entries().tobytes() == twin.group_trend_entries().tobytes()
    assert g.group_node_trend_entries().tobytes() == twin.group_node_trend_entries().tobytes()
    for call in (twin.window_group_incidents, twin.window_group_node_incident, twin.window_group_incidents_buffer):
        assert _rc(call) == engine.SG_ESTATE


# ---- 2. boundary shapes -------------------------------------------------------------------------------------------------------------
MG = 3000                                                             # max_groups: KNOWN ids 2999, 3000, 3001 lie on either side of it
N_PODS = 10_100
ALL = dict(by="score", min_value=-INF)                                # every group edge is red (a score is never NaN here)


@pytest.fixture(scope="module")
def big():
    """10 100 pods, max_edges 32 768: plan_group_incidents takes 256 workload rows per workgroup of k18_label / k18_number.
    Workload 5 = pods 0, 1; workloads 0 .. 2 = pods 2, 3, 4; everything else is ungrouped.  Every group edge red, K17 on"""
    topo = replay.make_topology(N_PODS, 4 * N_PODS, seed=7, svcs=4)
    mk = topo.n_nodes + 8
    g = engine.ServiceGraph(max_known_nodes=mk, max_edges=1 << 15, layers=2, max_labels=16, max_outbound_ips=64, max_window_events=1 << 16,
                            max_batch=1 << 14)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(2)
    g.set_groups(max_groups=MG); g.group_assign([0, 1, 2, 3, 4], [5, 5, 0, 1, 2])
    g.set_group_nodes(); g.set_group_rank(iters=2); g.set_group_incidents(**ALL)
    return topo, g, mk


def _all_red(g):
    return _check(g, "score", -INF, True)


def test_windows_of_no_and_of_one_group_edge_and_alive_only(big):
    topo, g, mk = big
    none = np.zeros(0, np.int64)
    _send(topo, g, none, none)
    assert len(_all_red(g)) == 0 and len(g.window_groups()) == 0 and len(g.window_group_node_incident()) == 0
    _send(topo, g, [0, 1], [1, 0])                                    # one group edge INSIDE workload 5: its row alone is an incident
    got = _all_red(g)
    assert len(g.window_groups()) == 1 and (got["nodes"][0], got["edges"][0], got["first_node"][0]) == (1, 1, 0)
    _send(topo, g, [9], [10])
    got = _all_red(g)
    assert (got["nodes"][0], got["edges"][0]) == (2, 1) and g.window_group_node_incident().tolist() == [0, 0]
    src = np.arange(100, 400); dst = 100 + (np.arange(300) * 7 + 1) % 300
    rows = _send(topo, g, src, dst, alive=np.ones(300, bool))         # alive-only group edges are ordinary group edges
    assert (rows["count"] == 0).all() and len(rows) == 300
    got = _all_red(g)
    assert int(got["edges"].sum()) == 300 and (got["count"] == 0).all()


@pytest.mark.parametrize("down", [False, True])
def test_one_chain_of_4097_pods(big, down):
    """ascending: pod i calls pod i + 1, every hook puts the larger row under the smaller; descending: pod i + 1 calls pod i.
    Either way one incident of 4097 rows whose root walks are long"""
    topo, g, mk = big
    a, b = np.arange(10, 10 + 4096), np.arange(11, 11 + 4096)
    _send(topo, g, b if down else a, a if down else b)
    got = _all_red(g)
    assert len(got) == 1 and (got["nodes"][0], got["edges"][0], got["first_node"][0]) == (4097, 4096, 0)
    assert (g.window_group_node_incident() == 0).all()


def test_64_disjoint_chains_and_two_chains_joined_by_the_last_group_edge(big):
    topo, g, mk = big
    src = np.concatenate([np.arange(100 * c + 10, 100 * c + 10 + 40) for c in range(64)])
    _send(topo, g, src, src + 1)
    got = _all_red(g)
    assert len(got) == 64 and (got["nodes"] == 41).all() and (got["edges"] == 40).all()
    assert got["first_node"].tolist() == [41 * c for c in range(64)]
    inc = g.window_group_node_incident()
    assert inc.tolist() == np.repeat(np.arange(64), 41).tolist()
    # chains 100 .. 199 and 300 .. 399; the group edge 399 -> 100 has the largest source: it is the last one, and joins them
    s = np.concatenate([np.arange(100, 199), np.arange(300, 399)])
    _send(topo, g, s, s + 1)
    assert _all_red(g)["nodes"].tolist() == [100, 100]
    _send(topo, g, np.concatenate([s, [399]]), np.concatenate([s + 1, [100]]))
    got = _all_red(g)
    ge = g.window_groups()
    assert (ge["from_ref"][-1], ge["to_ref"][-1]) == (399, 100)
    assert got["nodes"].tolist() == [200] and got["edges"].tolist() == [199]


def test_one_callee_and_one_caller_hold_5000_group_edges(big):
    """every CAS of the hook lands on one root"""
    topo, g, mk = big
    _send(topo, g, np.arange(100, 5100), np.full(5000, 7))
    got = _all_red(g)
    assert got["nodes"].tolist() == [5001] and got["edges"].tolist() == [5000] and got["first_node"].tolist() == [0]
    _send(topo, g, np.full(5000, 7), np.arange(100, 5100))
    got = _all_red(g)
    assert got["nodes"].tolist() == [5001] and got["edges"].tolist() == [5000]
    _send(topo, g, np.full(5000, 9000), np.arange(100, 5100))         # the one caller is the LARGEST row: every hook moves the root down
    got = _all_red(g)
    assert got["nodes"].tolist() == [5001] and got["first_node"].tolist() == [0]


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_row_counts_around_the_node_span(big, n):
    """n workload rows in pairs and one triple: incidents whose heads lie on either side of a workgroup's 256 rows"""
    topo, g, mk = big
    ids = 50 + np.arange(n)
    src = ids[:-1][::2] if n % 2 == 0 else np.concatenate([ids[:-1][::2], [ids[-2]]])
    dst = src + 1
    _send(topo, g, src, dst)
    got = _all_red(g)
    assert len(g.window_group_nodes()) == n and len(got) == n // 2
    assert got["first_node"].tolist() == list(range(0, 2 * (n // 2), 2))


def test_a_red_group_edge_inside_a_workload_beside_a_chain(big):
    topo, g, mk = big
    s = np.arange(200, 260)
    _send(topo, g, np.concatenate([[0, 1], s, [2]]), np.concatenate([[1, 0], s + 1, [200]]))   # workload 5 alone; workload 0 calls the chain
    got = _all_red(g)
    gn = g.window_group_nodes()
    assert gn["ref"][:2].tolist() == [G(0), G(5)]
    assert got["first_node"].tolist() == [0, 1] and got["nodes"].tolist() == [62, 1] and got["edges"].tolist() == [61, 1]


def test_label_obip_and_known_ids_on_either_side_of_max_groups(big):
    topo, g, mk = big
    rng = np.random.default_rng(3)
    ids = np.array([MG - 1, MG, MG + 1, 5, 6, 0, 1, 2, 3, 4])
    pod = _events(topo, np.concatenate([ids, rng.integers(0, 6000, 2000)]), topo.pod_ips[np.concatenate([np.roll(ids, 3), rng.integers(0, 6000, 2000)])],
                  status=np.where(np.arange(2010) % 5 == 0, 503, 200))
    ext = _events(topo, rng.integers(0, 6000, 300), EXT + rng.integers(0, 2, 300).astype(np.uint32), label=np.repeat([1, 2, 0], 100))
    g.ingest_bulk(np.concatenate([pod, ext]))
    g.flush_window()
    got = _all_red(g)
    gn, inc = g.window_group_nodes(), g.window_group_node_incident()
    assert {0, 1, 2, 3} == set((gn["ref"] >> 30).tolist())           # KNOWN, LABEL, OBIP and GROUP rows
    assert (inc != NO).all() and len(got) >= 1
    for ref in (MG - 1, MG, MG + 1, G(5), G(0)):
        assert (gn["ref"] == ref).any(), ref
    # the same window at a threshold that leaves some group edges out
    thr = quantile_threshold(g.window_groups()["score_max"], 0.9)
    g.set_group_incidents(by="score", min_value=thr)
    g.ingest_bulk(np.concatenate([pod, ext])); g.flush_window()
    cut = _check(g, "score", thr, True)
    g.set_group_incidents(**ALL)
    assert 0 < int(cut["edges"].sum()) < int(got["edges"].sum())


# ---- 3. the direct path -------------------------------------------------------------------------------------------------------------
def test_more_incidents_through_one_workgroup_than_its_table_has_slots():
    """max_edges 4096 over 8200 pods: 4096 disjoint red pairs 2i -> 2i + 1 are 4096 incidents; each of the four workgroups of
    k18_nodes takes 2048 rows and each of the four of k18_rows 1024 group edges — 1024 distinct incidents against 512 table slots
    (tests/test_group_incident_host.py holds the plan to that), and no wave names one incident"""
    topo = replay.make_topology(8200, 4 * 8200, seed=7, svcs=4)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=4096, layers=2, max_labels=16, max_outbound_ips=64,
                            max_window_events=1 << 16, max_batch=1 << 14)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    g.set_groups(); g.set_group_nodes(); g.set_group_rank(iters=2); g.set_group_incidents(**ALL)
    src = 2 * np.arange(4096)
    rows = _send(topo, g, src, src + 1)
    assert len(rows) == 4096
    got = _all_red(g)
    assert len(got) == 4096 and (got["nodes"] == 2).all() and (got["edges"] == 1).all()
    assert got["first_node"].tolist() == src.tolist() and got["worst_row"].tolist() == list(range(4096))
    assert g.window_group_node_incident().tolist() == np.repeat(np.arange(4096), 2).tolist()


# ---- 4. close paths -----------------------------------------------------------------------------------------------------------------
def test_every_close_path_gives_the_same_rows(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    g.set_group_trend(**TREND); g.set_group_nodes(); g.set_group_node_trend(shift=3, warmup=2, ttl=2); g.set_group_rank(iters=3)
    thr = 0.0
    for i, w in enumerate(wins[:7]):
        by = BYS[i % 3]
        g.set_group_incidents(by=by, min_value=thr)
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_group_incidents, g.window_group_node_incident, g.set_group_incidents):
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            assert _rc(g.set_group_incidents, None) == engine.SG_ESTATE
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
        ge, tr = g.window_groups(), g.window_group_trend()
        got = _check(g, by, thr, True, ge=ge, trend=tr)
        assert i == 0 or len(got) > 0
        thr = quantile_threshold(group_values(ge, BYS[(i + 1) % 3], tr), 0.9)


def test_window_run_in_flight_under_a_changing_map(churn):
    """sg_window_run with three windows in flight, the map changing between the closes: each window's incidents, read from the
    device buffers after the whole round was enqueued, against the reference over a one-call engine's group edges and workload
    rows and the in-flight engine's own rank rows"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=3), _engine(topo, labels)
    for x in (g, one):
        x.set_groups(); x.set_group_nodes()
    g.set_group_rank(iters=2)
    thr = None
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending, counts = [], []
    for i, w in enumerate(wins[:9]):
        lo = 30 * i
        for x in (g, one):
            x.group_assign(np.arange(lo, lo + 40), np.arange(lo, lo + 40) // (3 + i % 4))
        _feed(one, w)
        one.flush_window()
        ge, gn = one.window_groups(), one.window_group_nodes()
        if thr is None:                                               # (nothing is in flight yet: the switch may allocate)
            thr = quantile_threshold(ge["score_max"], 0.9)
            g.set_group_incidents(by="score", min_value=thr)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((ge, gn, g.window_group_rank_buffer(), g.window_group_incidents_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for ge, gn, rp, (ip, cp, np_) in pending:
                n_inc = int(_d2h(hip, cp, 1, np.uint64)[0])
                rank = _d2h(hip, rp, len(gn), engine.RANK_DTYPE)
                got = _d2h(hip, ip, n_inc, engine.INCIDENT_DTYPE) if n_inc else np.zeros(0, engine.INCIDENT_DTYPE)
                _check(g, "score", thr, True, ge=ge, gn=gn, rank=rank, got=got, ginc=_d2h(hip, np_, len(gn), np.uint32))
                counts.append(n_inc)
            pending = []
    assert len(counts) == 9 and max(counts) > 0


# ---- 5. lifecycle --------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    reads = (g.window_group_incidents, g.window_group_node_incident, g.window_group_incidents_buffer)
    assert _rc(g.set_group_incidents) == engine.SG_ESTATE and _rc(g.set_group_incidents, None) == engine.SG_ESTATE   # the groups are off
    g.set_groups(); g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7)
    assert _rc(g.set_group_incidents) == engine.SG_ESTATE              # the workload rows are off
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_group_nodes()
    assert _rc(g.window_group_incidents) == engine.SG_ESTATE           # the stage is off
    for bad in (dict(by=3), dict(by=7), dict(struct_size=12), dict(struct_size=20), dict(reserved=1)):
        assert _rc(g.set_group_incidents, **bad) == engine.SG_EINVAL
    for by in ("lat_dev", "err_dev"):
        assert _rc(g.set_group_incidents, by=by) == engine.SG_ESTATE   # a trend key without the group trend
    _feed(g, wins[0]); g.flush_window()
    g.set_group_incidents(min_value=0.5)
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE                           # the read window was closed while it was off
    _feed(g, wins[1]); g.flush_window()
    _check(g, "score", 0.5)
    n = len(g.window_group_nodes())
    inc = g.window_group_node_incident()
    # the index form: repeats, empty, out of range, longer than the staging (the slot's row capacity), a cap below the count
    rep = np.array([5, 5, 0, n - 1, 5], np.uint32)
    assert g.window_group_node_incident(rep).tolist() == inc[rep].tolist()
    assert len(g.window_group_node_incident(np.zeros(0, np.uint32))) == 0
    assert _rc(g.window_group_node_incident, np.array([0, n], np.uint32)) == engine.SG_EINVAL
    cap = g.window_buffers()[3] + topo.n_nodes + 8                     # GK = max_groups + the node capacity: at least the slot's row capacity
    long = (np.arange(cap + 1001) % n).astype(np.uint32)
    assert g.window_group_node_incident(long).tolist() == inc[long].tolist()
    out = np.full(5, 0xFFFFFFFF - 1, np.uint32)
    cnt = C.c_size_t(0)
    assert g._l.sg_window_group_node_incident(g._h, rep.ctypes.data, 5, out.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == 5 and out[:3].tolist() == inc[rep[:3]].tolist() and out[3:].tolist() == [0xFFFFFFFF - 1] * 2
    # what does not touch it: the map, K17, K9 / K11 / K12 / K13
    g.group_assign([0, 1], [5, NOG])
    g.set_group_rank(iters=2)
    g.set_nodes(); g.set_rank(iters=2); g.set_incidents(min_value=0.5); g.set_tracks(); g.set_tracks(None); g.set_incidents(None)
    _feed(g, wins[2]); g.flush_window()
    _check(g, "score", 0.5, True)
    g.set_group_rank(None); g.set_nodes(False)
    _feed(g, wins[3]); g.flush_window()
    _check(g, "score", 0.5)
    # the group trend: switching it off takes a trend-keyed stage with it, and leaves a score-keyed one
    g.set_group_trend(**TREND)
    g.set_group_incidents(by="lat_dev", min_value=0.0)
    assert _rc(g.window_group_incidents) == engine.SG_ESTATE           # new parameters: the windows from here on
    _feed(g, wins[4]); g.flush_window()
    _check(g, "lat_dev", 0.0)
    g.set_group_trend(**TREND)                                        # on again with parameters: the stage stays
    _feed(g, wins[5]); g.flush_window()
    _check(g, "lat_dev", 0.0)
    g.set_group_trend(None)
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_group_incidents(min_value=0.5)
    g.set_group_trend(**TREND); g.set_group_trend(None)
    _feed(g, wins[6]); g.flush_window()
    _check(g, "score", 0.5)
    g.set_group_incidents(None)
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_group_incidents(min_value=0.5)
    g.set_group_nodes(False)                                          # the workload rows off take the stage with them
    assert _rc(g.window_group_incidents) == engine.SG_ESTATE and _rc(g.set_group_incidents) == engine.SG_ESTATE
    g.set_group_nodes()
    _feed(g, wins[7]); g.flush_window()
    assert _rc(g.window_group_incidents) == engine.SG_ESTATE and len(g.window_group_nodes()) > 0
    g.set_group_incidents(min_value=0.5)                              # re-enabled
    _feed(g, wins[8]); g.flush_window()
    _check(g, "score", 0.5)
    g.set_groups()                                                    # any sg_set_groups call frees it
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE
    assert _rc(g.set_group_incidents) == engine.SG_ESTATE
    _feed(g, wins[9]); g.flush_window()
    assert len(g.window_groups()) > 0


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------
def test_the_workload_incident_keeps_its_names_through_a_rollout():
    """frontend (pods 0..2) -> checkout (3, 4) -> payments (5..8) beside steady traffic among ungrouped pods, keyed by lat_dev.  After
    K15's warm-up the chain slows down: one workload incident.  Then every pod of the chain is replaced (pods 10..18, the same
    groups) and the chain is still slow: the workload incident of that window has the same first_node ref, nodes, top_node ref and
    culprit ref.  K12 on the same engine, keyed by K8's lat_dev, names the old pods before the rollout and none of them after it:
    its baseline is keyed by pod"""
    topo, g, mk = _pods_engine()
    warmup, thr = 2, 3.0
    sizes = (3, 2, 4)

    def tiers(first):
        out, nxt = [], first
        for s in sizes:
            out.append(list(range(nxt, nxt + s))); nxt += s
        return out
    g.set_groups()
    for first in (0, 10):
        for grp, tier in enumerate(tiers(first)):
            g.group_assign(tier, [grp] * len(tier))
    g.set_group_trend(shift=3, warmup=warmup); g.set_group_nodes(); g.set_group_rank()
    g.set_group_incidents(by="lat_dev", min_value=thr)
    g.set_trend(shift=3, warmup=warmup); g.set_nodes(); g.set_incidents(by="lat_dev", min_value=thr)
    other_s, other_d = _pairs(40, 60, 3)                              # steady traffic among ungrouped pods 30..69

    def close(first, dur):
        ids = tiers(first)
        src = [a for up, down in zip(ids, ids[1:]) for a in up for _ in down]
        dst = [b for up, down in zip(ids, ids[1:]) for _ in up for b in down]
        d = np.concatenate([np.full(len(src), dur), np.full(60, 1_000_000)])
        _send(topo, g, np.concatenate([src, other_s + 30]), np.concatenate([dst, other_d + 30]), dur=d)
        return _check(g, "lat_dev", thr, True)
    for _ in range(warmup + 2):
        assert len(close(0, 1_000_000)) == 0 and len(g.window_incidents()) == 0
    seen = []
    for first, dur in ((0, 5_000_000), (10, 25_000_000)):
        got = close(first, dur)
        gn = g.window_group_nodes()
        assert len(got) == 1 and got["nodes"][0] == 3 and got["edges"][0] == 2
        o = got[0]
        assert gn["ref"][:3].tolist() == [G(0), G(1), G(2)]
        pods = g.window_nodes()["ref"][g.window_node_incident() != NO]
        seen.append(((int(gn["ref"][o["first_node"]]), int(o["nodes"]), int(gn["ref"][o["top_node"]]), int(gn["ref"][o["culprit_node"]])),
                     set(pods.tolist())))
    assert seen[0][0] == seen[1][0] and seen[0][0][0] == G(0)          # the same workloads under the same names
    assert seen[0][1] == set(range(9)) and not (seen[1][1] & seen[0][1])   # K12: the old pods, then none of them
