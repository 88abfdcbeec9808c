"""K25, the replica outliers (sg_set_replicas / sg_window_replicas / sg_window_group_replicas / sg_window_replicas_buffer /
sg_window_replicas_top): the pod rows and the workload rows after every window against tests/replica_ref.py — byte for byte — run on
the same engine's own node rows, workload rows and K20 node histograms of that window, under the map the window was contracted
under.  Windows are a few hundred to a few thousand events: the churn of tests/traces.py thinned, and a constructed pod-to-pod
window whose sizes are held to the plan (tests/micro/replica_plan_test.cpp)."""
import ctypes as C
from collections import Counter
import json
import os
import subprocess

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import EXT, _d2h, _engine, _events, _feed, _hip, _map, _ncap, _rc
from tests.helpers import CLOCK, HostShim
from tests.replica_ref import (CHURN_COUNTS, CHURN_PARAMS, CHURN_STEP, CHURN_WINDOWS, ERR, JUDGED, LAT, MEMBER, NONE, SIDES, TAIL, ref_select_replicas, replica_ref,
                               replica_values, tally)
from tests.traces import churn  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_GROUP
PARAMS = CHURN_PARAMS                                                 # (tests/test_replicas_churn.py: non-vacuous by the reference alone, on the CPU)


class _Quiet:
    upsert_pod = upsert_service = delete_pod = delete_service = staticmethod(lambda *a: None)


def _kinds(topo, mk):
    """the kind per KNOWN id and the ids of the Services, as HostShim interns the topology"""
    sh = HostShim(); sh.apply(_Quiet(), topo.k8s_ops())
    k = np.zeros(mk, np.uint8)
    k[:len(sh.kind)] = [1 if x == "pod" else 2 for x in sh.kind]
    return k, [i for i, x in enumerate(sh.kind) if x == "service"]


def _stages(g, gmap, tails=True):
    g.set_nodes(); g.set_groups()
    g.group_assign(np.arange(len(gmap)), gmap)
    g.set_group_nodes()
    if tails:
        g.set_quantiles(("nodes",))


def _thin(w, step=CHURN_STEP):
    return w[::step]


def _want(g, gmap, kinds, params):
    nodes, wrows = g.window_nodes(), g.window_group_nodes()
    hist = g.window_node_hist() if params.get("tail_permille") else None
    return nodes, wrows, replica_ref(nodes, wrows, hist, gmap, kinds, params)


def _check(g, gmap, kinds, params):
    """the last read window's rows against the reference over the engine's own rows of that window; returns them"""
    nodes, wrows, (want_p, want_g) = _want(g, gmap, kinds, params)
    got_p, got_g = g.window_replicas(), g.window_group_replicas()
    assert got_p.shape == want_p.shape and got_g.shape == want_g.shape, (got_p.shape, want_p.shape, got_g.shape, want_g.shape)
    bad = np.flatnonzero((got_p != want_p).any(axis=1))
    assert got_p.tobytes() == want_p.tobytes(), (bad[:4].tolist(), got_p[bad[:2]].tolist(), want_p[bad[:2]].tolist())
    bad = np.flatnonzero((got_g != want_g).any(axis=1))
    assert got_g.tobytes() == want_g.tobytes(), (bad[:4].tolist(), got_g[bad[:2]].tolist(), want_g[bad[:2]].tolist())
    return nodes, wrows, got_p, got_g


def _twin_reads(g):
    calls = ["window_nodes", "window_groups", "window_group_nodes", "window_group_perm", "window_hist", "window_node_hist", "window_node_quantiles"]
    return {c: getattr(g, c)().tobytes() for c in calls}


# ---- 1. the churn: exact after every window, a twin without the stage unchanged ------------------------------------------------------
def test_churn_is_exact_and_a_twin_without_the_stage_is_unchanged(churn):
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    kinds, _ = _kinds(topo, mk)
    g, twin = (_engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True) for _ in range(2))
    for x in (g, twin):
        _stages(x, gmap)
    g.set_replicas(**PARAMS)
    t = None
    for w in wins[:CHURN_WINDOWS]:
        _feed(g, _thin(w)); _feed(twin, _thin(w))
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        a, b = _twin_reads(g), _twin_reads(twin)
        for c in a:
            assert a[c] == b[c], c
        _, _, pods, groups = _check(g, gmap, kinds, PARAMS)
        t = tally(pods, t)
    print("churn:", t)
    assert all(v > 0 for v in t.values()), t                          # nothing here passes vacuously
    assert t == CHURN_COUNTS, t                                       # the counts the reference finds over the oracle's edges, without an engine


# ---- 2. the constructed window -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replica_plan") / "replica_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "micro", "replica_plan_test.cpp")])

    def run(ncap, gk, nc, tail):
        line = f"1 15 {ncap} {gk} {nc} 1 40 0 0 0 0 {tail} 0 0 0\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return json.loads(out.stdout)
    return run


N_PODS, MK = 900, 4200
BIG = np.arange(100, 400)                                             # workload 0: three hundred replicas
SINGLES = np.arange(400, 640)                                         # workloads 10 .. 249: one pod each
CLIENTS = np.arange(850, 900)                                         # ungrouped
CON = dict(min_replicas=3, min_requests=20)


def _pods(**kw):
    topo = replay.make_topology(N_PODS, 4 * N_PODS, seed=7, svcs=4)    # (the pods, their ids and one Service are used)
    g = engine.ServiceGraph(max_known_nodes=MK, max_edges=1 << 13, layers=2, max_labels=16, max_outbound_ips=64, max_window_events=1 << 16,
                            max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(16)
    kinds, svcs = _kinds(topo, MK)
    assert (kinds[:N_PODS] == 1).all() and len(svcs) == 4             # pod i has node id i
    return topo, g, kinds, svcs


def _constructed_map(svcs):
    m = np.full(MK, NO, np.uint32)
    m[BIG] = 0
    m[0:4] = 1; m[4:7] = 2; m[7:10] = 3; m[10:14] = 4; m[14:18] = 5; m[svcs] = 5; m[20:24] = 6   # service binding: the Services beside workload 5's pods
    m[SINGLES] = 10 + np.arange(len(SINGLES))
    m[640:644] = 250
    return m


def _constructed_events(topo, svc_ip):
    ev = []
    def to(src, dst, n, **kw):
        ev.append(_events(topo, np.repeat(src, n), topo.pod_ips[np.repeat(dst, n)], **kw))
    for i, p in enumerate(BIG):                                       # twenty requests each; replica 137 is slow, replica 311 fails
        to(CLIENTS[i % 50], p, 20, dur=1 << (23 if p == 137 else 20), status=503 if p == 311 else 200)
    for p in range(4):                                                # workload 1 calls pod 840: replica 0 is an error outlier on the out side only
        to(p, 840, 25, status=[503] * 10 + [200] * 15 if p == 0 else 200)
    for p in (4, 5, 6):                                               # workload 2: min_replicas active members
        to(CLIENTS[p], p, 20)
    for p in (7, 8):                                                  # workload 3: min_replicas - 1 active on the in side; pod 9 only sends
        to(CLIENTS[p], p, 20)
    to(9, 841, 1)
    for p, n in ((10, 19), (11, 20), (12, 20), (13, 20)):            # workload 4: a member at min_requests - 1 and one at min_requests
        to(CLIENTS[p], p, n)
    for p in range(14, 18):                                           # workload 5: four pods and the bound Service beside them
        to(CLIENTS[p], p, 20)
    ev.append(_events(topo, np.repeat(CLIENTS[0], 30), np.full(30, svc_ip, np.uint32)))
    for p in range(20, 24):                                           # workload 6: replica 20 is a tail-only outlier, 3 % two octaves up
        to(CLIENTS[p], p, 100, dur=[1 << 20] * 97 + [1 << 22] * 3 if p == 20 else 1 << 20)
    for i, p in enumerate(SINGLES):
        to(CLIENTS[i % 50], p, 1)
    for p in range(640, 644):                                         # workload 250: beyond the first range; replica 640 is slow
        to(CLIENTS[p % 50], p, 20, dur=1 << (23 if p == 640 else 20))
    ev.append(_events(topo, [845, 846, 847, 847], EXT + np.arange(4, dtype=np.uint32), label=[1, 16, 0, 0]))   # LABEL and OBIP nodes
    return np.concatenate(ev)


@pytest.mark.parametrize("tail", [990, 0])
def test_the_constructed_window(plan, tail):
    topo, g, kinds, svcs = _pods(edge_histogram=bool(tail))           # tails off: the stage runs without SG_CFG_EDGE_HISTOGRAM
    gmap = _constructed_map(svcs)
    _stages(g, gmap, tails=bool(tail))
    params = dict(CON, tail_permille=tail)
    g.set_replicas(**params)
    g.ingest_bulk(_constructed_events(topo, topo.svc_ips[0])); g.flush_window()
    nodes, wrows, pods, groups = _check(g, gmap, kinds, params)
    # The engine exposes its node capacity, not K16's sizes; they follow from it as include/servicegraph.h ("groups") and
    # plan_group_nodes state them: GK = max_groups + the node capacity with max_groups = max_known_nodes (sg_set_groups' default,
    # which _stages takes), and min(GK, 2 x max_edges) workload rows a slot.  plan_replicas reads nothing else of the engine.
    ncap = _ncap(g)
    assert ncap == MK + 16 + 64                                       # max_known_nodes + max_labels + max_outbound_ips
    gk = MK + ncap
    P = plan(ncap, gk, min(gk, 2 << 13), tail)
    assert P["rc"] == 0 and P["slices"] > 1 and len(wrows) <= P["nc"] and len(nodes) <= P["ncap"]
    if tail:
        assert len(wrows) > P["range_rows"]                           # more workload rows than one range holds
    else:
        assert len(wrows) <= P["range_rows"]                          # (tails off: 1024 rows a range, one range here; the tails-on case has several)
    refs = nodes["ref"].tolist()
    at = {r: k for k, r in enumerate(refs)}
    per = -(-len(nodes) // P["slices"])
    assert len({at[int(p)] // per for p in BIG}) > 1                  # workload 0's members span more than one slice
    row = lambda p: pods[at[p]].tolist()
    w_of = {int(r) & 0x3FFFFFFF: k for k, r in enumerate(wrows["ref"].tolist()) if int(r) >> 30 == 3}
    assert row(137)[0] == w_of[0] and row(137)[1] == MEMBER | JUDGED | LAT | (TAIL if tail else 0) and row(137)[6] == 300
    assert row(311)[1] == MEMBER | JUDGED | ERR and row(100)[1] == MEMBER | JUDGED and row(100)[4] == 1024
    assert groups[w_of[0]].tolist()[:4] == [300, 300, 2, at[137]]
    assert row(0)[1] == MEMBER | (JUDGED | ERR) << 4 and row(1)[1] == MEMBER | JUDGED << 4      # the out side only
    assert groups[w_of[1]].tolist() == [0, 0, 0, NONE, 4, 4, 1, at[0]]
    assert [row(p)[1] for p in (4, 5, 6)] == [MEMBER | JUDGED] * 3 and [row(p)[1] for p in (7, 8, 9)] == [MEMBER] * 3
    assert groups[w_of[3]].tolist()[:4] == [2, 0, 0, NONE]
    assert row(10)[1] == MEMBER and row(11)[1] == MEMBER | JUDGED
    bound = [r for r in refs if r < MK and kinds[r] == 2]             # the Service the clients called
    assert len(bound) == 1 and row(bound[0]) == [NONE] + [0] * 11 and row(14)[6] == 4 and groups[w_of[5]].tolist()[:2] == [4, 4]
    assert int(wrows[w_of[5]]["in_count"]) == 4 * 20 + 30             # the Service's traffic is the workload's, not a member's
    assert row(20)[1] == MEMBER | JUDGED | (TAIL if tail else 0) and row(20)[3] < 2048 and row(20)[5] == (6 | 4 << 8 if tail else 0)
    assert w_of[250] > (P["range_rows"] if tail else 0) and row(640)[1] & LAT and groups[w_of[250]].tolist()[:4] == [4, 4, 1, at[640]]
    for r in (845, 850, 840, 1 << 30 | 0, 1 << 30 | 15):              # ungrouped pods and LABEL nodes
        assert row(r) == [NONE] + [0] * 11, r
    ob = (nodes["ref"] >> 30) == 2
    assert ob.sum() == 2 and (pods[ob, 0] == NONE).all() and (pods[ob, 1:] == 0).all()
    if not tail:
        assert (pods[:, 5] == 0).all() and (pods[:, 10] == 0).all()   # the tail words


# ---- 3. a regrouping between windows ------------------------------------------------------------------------------------------------------
def test_each_window_is_judged_under_the_map_it_was_contracted_under():
    topo, g, kinds, svcs = _pods(edge_histogram=True)
    gmap = _constructed_map(svcs)
    _stages(g, gmap)
    params = dict(CON, tail_permille=990)
    g.set_replicas(**params)
    ev = _constructed_events(topo, topo.svc_ips[0])
    g.ingest_bulk(ev); g.flush_window()
    _, _, before, _ = _check(g, gmap, kinds, params)
    moved = gmap.copy()
    moved[137] = 2; moved[4] = NO; moved[0:4] = 3                     # the slow replica joins workload 2; workloads 1 and 3 merge
    g.group_assign(np.array([137, 4, 0, 1, 2, 3]), moved[[137, 4, 0, 1, 2, 3]])
    g.ingest_bulk(ev); g.flush_window()
    nodes, wrows, after, groups = _check(g, moved, kinds, params)
    at = {r: k for k, r in enumerate(nodes["ref"].tolist())}
    assert after[at[137], 0] != before[at[137], 0] and after[at[137], 6] == 3 and after[at[4], 0] == NONE
    assert after[at[0], 1] == MEMBER | (JUDGED | ERR) << 4 and after[at[7], 11] == 5     # pods 0 .. 3 and 9 send; pods 7 and 8 are their siblings now
    g.set_replicas(**params)                                          # sg_group_assign does not touch the stage; a new set starts the same
    g.ingest_bulk(ev); g.flush_window()
    _check(g, moved, kinds, params)


# ---- 4. every close path, and three windows in flight -------------------------------------------------------------------------------------
def test_every_close_path(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    kinds, _ = _kinds(topo, mk)
    _stages(g, gmap)
    g.set_trend(shift=3, warmup=1)                                    # (for the _top_by flush)
    g.set_replicas(**PARAMS)
    for i, w in enumerate(wins[:8]):
        _feed(g, _thin(w))
        if i == 0:
            g.flush_begin()
            for call in (g.window_replicas, g.window_group_replicas, g.set_replicas):
                assert _rc(call) == engine.SG_ESTATE                  # a flush is open
            assert _rc(g.window_replicas_top, 1) == engine.SG_ESTATE
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
        elif i == 6:
            g.flush_window_top(2, by="lat_dev")                       # sg_flush_window_top_by
        else:
            g.flush_begin(); g.flush_end_top(2)
        _check(g, gmap, kinds, PARAMS)


def test_window_run_three_in_flight_through_the_device_buffers(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True, windows_in_flight=3)
    one = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    kinds, _ = _kinds(topo, mk)
    for x in (g, one):
        _stages(x, gmap)
        x.set_replicas(**PARAMS)
    hip = _hip()
    thin = [np.ascontiguousarray(_thin(w)) for w in wins[:6]]
    dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in thin]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(thin):
        if i in (2, 4):                                               # a regrouping while windows are in flight: each under its own map
            gmap = gmap.copy(); gmap[:21] = (gmap[:21] + i) % 3
            for x in (g, one):
                x.group_assign(np.arange(21), gmap[:21])
        _feed(one, w)
        one.flush_window()
        _, _, want_p, want_g = _check(one, gmap, kinds, PARAMS)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((want_p, want_g, g.window_replicas_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for want_p, want_g, (pp, pg) in pending:
                assert _d2h(hip, pp, want_p.nbytes, np.uint8).tobytes() == want_p.tobytes()
                assert _d2h(hip, pg, want_g.nbytes, np.uint8).tobytes() == want_g.tobytes()
                sizes.append(len(want_p))
            pending = []
    assert len(sizes) == 6 and len(set(sizes)) > 1


# ---- 5. the selection ----------------------------------------------------------------------------------------------------------------------
def test_the_selection_against_the_reference_for_every_key():
    topo, g, kinds, svcs = _pods(edge_histogram=True)
    gmap = _constructed_map(svcs)
    _stages(g, gmap)
    params = dict(CON, tail_permille=990)
    g.set_replicas(**params)
    g.ingest_bulk(_constructed_events(topo, topo.svc_ips[0])); g.flush_window()
    nodes, _, pods, _ = _check(g, gmap, kinds, params)
    for by in engine.RSEL_BY:
        for side in SIDES:
            vals = np.array(replica_values(pods, by, side))
            if by in ("share", "lat") or side == "in":
                assert (vals > 0).any(), (by, side)
            top = int(vals.max())
            tie = Counter(vals[vals > 0].tolist()).most_common(1)[0][0] if (vals > 0).any() else 1
            above = int((vals > tie).sum())
            for k, thr in ((0, 0), (0, tie), (0, top + 1), (1, 0), (above + 2, 0), (above + 2, tie), (len(nodes) + 5, 1)):   # above + 2: inside the tie
                want = ref_select_replicas(pods, by, side, k, thr)
                got, idx, n = g.window_replicas_top(k, thr, by=by, side=side)
                assert n == len(nodes) and idx.tolist() == want.tolist(), (by, side, k, thr)
                assert got.tobytes() == nodes[want].tobytes()
    want = ref_select_replicas(pods, "share", "in", 0, 0)             # cap < n_selected: the count is whole, cap rows are written
    cap = 5
    out, idx = np.zeros(cap, engine.NODE_DTYPE), np.zeros(cap, np.uint32)
    ns, nt = C.c_size_t(0), C.c_size_t(0)
    by = engine.RSEL_BY["share"] | engine.RSEL_SIDE["in"]
    assert g._l.sg_window_replicas_top(g._h, by, 0, 0, out.ctypes.data, idx.ctypes.data, cap, C.byref(ns), C.byref(nt)) == 0
    assert len(want) > cap and ns.value == len(want) and nt.value == len(nodes)
    assert idx.tolist() == want[:cap].tolist() and out.tobytes() == nodes[want[:cap]].tobytes()
    for bad in (0, 3, 4 | 8, 16 | 4, 1 | 12):                         # no side, both sides, an unknown bit
        assert g._l.sg_window_replicas_top(g._h, bad, 1, 0, None, None, 0, None, None) == engine.SG_EINVAL
    assert g._l.sg_window_replicas_top(g._h, 4, engine.SELECT_MAX_K + 1, 0, None, None, 0, None, None) == engine.SG_EINVAL


# ---- 6. lifecycle and return codes ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    kinds, _ = _kinds(topo, mk)
    plain = {k: v for k, v in PARAMS.items() if k != "tail_permille"}
    assert _rc(g.set_replicas, **plain) == engine.SG_ESTATE           # nothing upstream is on
    g.set_nodes()
    assert _rc(g.set_replicas, **plain) == engine.SG_ESTATE
    g.set_groups(); g.group_assign(np.arange(mk), gmap)
    assert _rc(g.set_replicas, **plain) == engine.SG_ESTATE           # the workload rows are off
    g.set_group_nodes()
    assert _rc(g.set_replicas, **PARAMS) == engine.SG_ESTATE          # tails without K20's node space
    g.set_quantiles(("group_nodes",))
    assert _rc(g.set_replicas, **PARAMS) == engine.SG_ESTATE          # ... another space does not serve
    for bad in (dict(min_replicas=1), dict(min_err_excess_q20=(1 << 20) + 1), dict(tail_permille=1000), dict(min_tail_bins=16), dict(reserved=1),
                dict(reserved=(0, 1))):
        assert _rc(g.set_replicas, **{**plain, **bad}) == engine.SG_EINVAL, bad
    for call in (g.window_replicas, g.window_group_replicas, g.window_replicas_buffer):
        assert _rc(call) == engine.SG_ESTATE                          # off
    assert _rc(g.window_replicas_top, 1) == engine.SG_ESTATE
    _feed(g, _thin(wins[0])); g.flush_window()
    g.set_replicas(**plain)
    assert _rc(g.window_replicas) == engine.SG_ESTATE                 # the last read window was closed while the stage was off
    assert _rc(g.window_replicas_top, 1) == engine.SG_ESTATE and _rc(g.window_replicas_buffer) == engine.SG_ESTATE
    _feed(g, _thin(wins[1])); g.flush_window()
    nodes, wrows, pods, groups = _check(g, gmap, kinds, plain)
    assert _rc(g.window_replicas, np.array([len(nodes)], np.uint32)) == engine.SG_EINVAL
    assert _rc(g.window_group_replicas, np.array([len(wrows)], np.uint32)) == engine.SG_EINVAL
    idx = np.array([3, 0, 3], np.uint32)
    assert g.window_replicas(idx).tobytes() == pods[idx].tobytes() and g.window_group_replicas(idx).tobytes() == groups[idx].tobytes()
    g.set_quantiles(("nodes",), (990, 500))                           # tails off: sg_set_quantiles leaves the stage alone
    _check(g, gmap, kinds, plain)
    g.set_replicas(**PARAMS)
    _feed(g, _thin(wins[2])); g.flush_window()
    _check(g, gmap, kinds, PARAMS)
    g.set_quantiles(("nodes",), (990, 500))                           # tails on: ANY sg_set_quantiles frees the stage in front of K20's tables
    assert _rc(g.window_replicas) == engine.SG_ESTATE
    g.set_replicas(**PARAMS); g.set_replicas(None)                    # off
    assert _rc(g.window_group_replicas) == engine.SG_ESTATE
    for off in (lambda: g.set_group_nodes(False), lambda: g.set_groups(), lambda: g.set_nodes(False)):
        g.set_nodes(); g.set_groups(); g.group_assign(np.arange(mk), gmap); g.set_group_nodes()
        g.set_replicas(**plain)
        _feed(g, _thin(wins[3])); g.flush_window()
        g.window_replicas()
        off()                                                         # an input freed underneath: the stage goes first
        assert _rc(g.window_replicas) == engine.SG_ESTATE and _rc(g.window_replicas_buffer) == engine.SG_ESTATE
