"""K19, the workload tracks (sg_set_group_tracks / sg_window_group_incident_tracks / sg_window_group_tracks_ended /
sg_window_group_tracks_buffer / sg_group_track_entries / sg_group_track_stats_get): the rows, the ended list, the table and the
counters of every window against the pure-Python reference tests/group_track_ref.py fed with the engine's own workload rows, workload
incident rows and incident per workload row of the same window — byte for byte, every field is an integer; under the map that groups
nothing against K13 on the same engine; a rollout through which the workload incident keeps its track while K13 opens new ones; a
regrouping between windows in flight; the shapes at which the kernels take another path; every close path; a twin without the stage;
and the lifecycle."""
import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _d2h, _engine, _events, _feed, _grouped, _hip, _rc, _send
from tests.group_track_ref import GroupTrackRef
from tests.helpers import CLOCK, G, HostShim
from tests.incident_ref import quantile_threshold
from tests.traces import churn  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

INF = float("inf")
NO = engine.NO_TRACK
NOG = engine.NO_GROUP
NEW, SPLIT, MERGED = engine.TRACK_NEW, engine.TRACK_SPLIT, engine.TRACK_MERGED
TREND = dict(shift=3, warmup=2, ttl=4)
ALL = dict(by="score", min_value=-INF)                                # every group edge is red (a score is never NaN here)
EXT = 0x5DB8D800                                                      # addresses outside the cluster
LABEL, OBIP = 1 << 30, 2 << 30


def _nc(g, max_groups):
    """the workload rows' capacity: min(max_groups + the node capacity, 2 x max_edges)"""
    return min(max_groups + g.window_buffers()[3], 2 * g.max_edges)


def _step(g, ref):
    """the reference's step over the last read window's own workload rows, incident per row and incident rows"""
    nodes, inc, ninc = g.window_group_nodes(), g.window_group_incidents(), g.window_group_node_incident()
    return ref.step(nodes, ninc, inc) + (inc,)


def _err(call, *a, **kw):
    """(the code, the library's text) of a call that fails"""
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(*a, **kw)
    return ei.value.rc, str(ei.value).split(": ", 1)[1]


def _check(g, ref):
    """the last read window's track rows, ended list, the table after it and the counters against the reference"""
    want, wended, inc = _step(g, ref)
    got, ended = g.window_group_incident_tracks(), g.window_group_tracks_ended()
    assert len(got) == len(want) == len(inc)
    assert got.tobytes() == want.tobytes(), (ref.w - 1, got.tolist(), want.tolist())
    assert ended.tobytes() == wended.tobytes(), (ref.w - 1, ended.tolist(), wended.tolist())
    assert g.group_track_entries().tobytes() == ref.entries().tobytes(), ref.w - 1
    s = g.group_track_stats()
    assert dict(windows=s.windows, live=s.live, opened=s.opened, dropped_cap=s.dropped_cap) == ref.stats()
    return got, ended


# ---- 1. the churn --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
@pytest.mark.parametrize("quiet", [0, 2])
@pytest.mark.parametrize("by", ["score", "lat_dev"])
def test_every_window_of_the_churn_is_exact(churn, kind, quiet, by):
    """K17 on; the threshold: fixed, the 0.9 quantile of a twin's window"""
    topo, labels, wins = churn
    (twin, _, mk), (g, _, _) = _grouped(topo, labels, kind), _grouped(topo, labels, kind)
    for x in (twin, g):
        x.set_group_trend(**TREND); x.set_group_nodes(); x.set_group_rank(iters=3)
    for w in wins[:1 if by == "score" else 4]:
        _feed(twin, w); twin.flush_window()
    thr = quantile_threshold(twin.window_groups()["score_max"] if by == "score" else twin.window_group_trend()[by], 0.9)
    g.set_group_incidents(by=by, min_value=thr)
    g.set_group_tracks(quiet_windows=quiet)
    ref = GroupTrackRef(quiet, 0, ncap=_nc(g, mk))
    flags, continued = 0, 0
    for w in wins:
        _feed(g, w); g.flush_window()
        got, _ = _check(g, ref)
        flags |= int(np.bitwise_or.reduce(got["flags"])) if len(got) else 0
        continued += int(((got["flags"] & NEW) == 0).sum())
    assert flags & NEW and continued > 0 and g.group_track_stats().opened > 0


# ---- 2. the identity map: K13 and K19 on one engine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("quiet,max_tracks", [(2, 0), (1, 6)])
def test_under_a_map_that_groups_nothing_it_is_k13(churn, quiet, max_tracks):
    topo, labels, wins = churn
    g, _, mk = _grouped(topo, labels, "none")
    g.set_nodes(); g.set_group_nodes()
    _feed(g, wins[0])
    thr = quantile_threshold(g.flush_window()["score"], 0.9)
    g.set_incidents(min_value=thr); g.set_group_incidents(min_value=thr)
    g.set_tracks(quiet_windows=quiet, max_tracks=max_tracks); g.set_group_tracks(quiet_windows=quiet, max_tracks=max_tracks)
    rows = 0
    for w in wins[1:]:
        _feed(g, w); g.flush_window()
        assert g.window_group_incidents().tobytes() == g.window_incidents().tobytes()
        a, b = g.window_incident_tracks(), g.window_group_incident_tracks()
        assert len(a) > 0 and a.tobytes() == b.tobytes()
        assert g.window_tracks_ended().tobytes() == g.window_group_tracks_ended().tobytes()
        assert g.track_entries().tobytes() == g.group_track_entries().tobytes()
        s, t = g.track_stats(), g.group_track_stats()
        assert (s.windows, s.live, s.opened, s.dropped_cap) == (t.windows, t.live, t.opened, t.dropped_cap)
        rows += len(a)
    assert rows > 0 and (max_tracks != 0 or g.group_track_stats().dropped_cap == 0)


# ---- constructed windows: pod-to-pod events and min_value = -inf, so a window's incidents are exactly the components fed -------------
def _pods(n_pods, max_edges=1 << 14, max_groups=0, in_flight=None, labels=0):
    topo = replay.make_topology(n_pods, 4 * n_pods, seed=7, svcs=4)    # (only the pods and their ids are used)
    mk = topo.n_nodes + 8
    kw = dict(windows_in_flight=in_flight) if in_flight else {}
    g = engine.ServiceGraph(max_known_nodes=mk, max_edges=max_edges, layers=2, max_labels=16, max_outbound_ips=64, max_window_events=1 << 16,
                            max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(labels)
    g.set_groups(max_groups=max_groups)
    return topo, g, mk, max_groups or mk


def _tracked(n_pods, quiet=2, max_tracks=0, grouped=0, **kw):
    """an engine over n_pods pods whose first `grouped` pods are each a workload of their own (pod i = workload i: GROUP refs), the
    others ungrouped (KNOWN refs); every group edge red"""
    topo, g, mk, mg = _pods(n_pods, **kw)
    if grouped:
        g.group_assign(np.arange(grouped), np.arange(grouped))
    g.set_group_nodes(); g.set_group_incidents(**ALL)
    g.set_group_tracks(quiet_windows=quiet, max_tracks=max_tracks)
    return topo, g, GroupTrackRef(quiet, max_tracks, ncap=_nc(g, mg))


def _window(topo, g, ref, pairs):
    """close a window of one request per (src pod, dst pod) pair (none: an empty window); (track rows, ended, incident rows)"""
    src, dst = (np.array(x, dtype=np.int64) for x in (zip(*pairs) if len(pairs) else ((), ())))
    assert len(_send(topo, g, src, dst)) == len(pairs)
    got, ended = _check(g, ref)
    return got, ended, g.window_group_incidents()


def _chain(ids):
    ids = [int(x) for x in ids]
    return list(zip(ids[:-1], ids[1:]))


# ---- 3. the rollout --------------------------------------------------------------------------------------------------------------------
def test_the_workload_incident_keeps_its_track_through_a_rollout():
    """frontend (pods 0..2) -> checkout (3, 4) -> payments (5..8), every pod in a Deployment.  Then every pod is replaced (pods
    10..18, the same groups): K19's incident keeps its track, every workload kept; K13 on the same engine opens new tracks"""
    topo, g, mk, _ = _pods(40)
    sizes = (3, 2, 4)

    def tiers(first):
        out, nxt = [], first
        for s in sizes:
            out.append(list(range(nxt, nxt + s))); nxt += s
        return out
    for first in (0, 10):
        for grp, tier in enumerate(tiers(first)):
            g.group_assign(tier, [grp] * len(tier))
    g.set_group_nodes(); g.set_group_incidents(**ALL); g.set_group_tracks(quiet_windows=0)
    g.set_nodes(); g.set_incidents(**ALL); g.set_tracks(quiet_windows=0)
    ref = GroupTrackRef(0, 0, ncap=_nc(g, mk))

    def close(first):
        ids = tiers(first)
        src = [a for up, down in zip(ids, ids[1:]) for a in up for _ in down]
        dst = [b for up, down in zip(ids, ids[1:]) for _ in up for b in down]
        _send(topo, g, src, dst)
        got, _ = _check(g, ref)
        assert len(got) == 1 and g.window_group_nodes()["ref"].tolist() == [G(0), G(1), G(2)]
        return got[0], g.window_group_incidents()[0], g.window_incident_tracks()
    for w in range(2):
        r, inc, pods = close(0)
        assert (r["track"], r["windows"], r["flags"]) == (0, w + 1, NEW if w == 0 else 0)
        assert len(pods) == 1 and (pods[0]["track"], pods[0]["flags"]) == (0, NEW if w == 0 else 0)
    r, inc, pods = close(10)                                          # the rollout
    assert (r["track"], r["parent"], r["windows"], r["flags"]) == (0, NO, 3, 0) and r["flags"] & NEW == 0
    assert r["kept_nodes"] == inc["nodes"] == 3 and (r["moved_nodes"], r["joined_nodes"]) == (0, 0)
    assert len(pods) == 1 and (pods[0]["track"], pods[0]["parent"], pods[0]["flags"], pods[0]["joined_nodes"]) == (1, NO, NEW, 9)
    assert g.window_tracks_ended()["track"].tolist() == [0] and len(g.window_group_tracks_ended()) == 0


# ---- 4. a regrouping between windows in flight -----------------------------------------------------------------------------------------
def test_window_run_in_flight_under_a_changing_map(churn):
    """sg_window_run with three windows in flight, sg_group_assign between the closes: each window's rows and ended list, read from
    the device buffers after the whole round was enqueued, against the reference over a one-call engine's workload rows and the
    in-flight engine's own incidents; the state updated in window order"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=3), _engine(topo, labels)
    for x in (g, one):
        x.set_groups(); x.set_group_nodes()
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    ref, pending, seen = None, [], 0
    for i, w in enumerate(wins[:9]):
        lo = 30 * i
        for x in (g, one):
            x.group_assign(np.arange(lo, lo + 40), np.arange(lo, lo + 40) // (3 + i % 4))
            if i % 3 == 2:
                x.group_assign(np.arange(0, lo, 5), NOG)              # some pods leave their workloads
        _feed(one, w)
        one.flush_window()
        gn = one.window_group_nodes()
        if ref is None:                                               # (nothing is in flight yet: the switches may allocate)
            g.set_group_incidents(by="score", min_value=quantile_threshold(one.window_groups()["score_max"], 0.9))
            g.set_group_tracks(quiet_windows=1)
            ref = GroupTrackRef(1, 0, ncap=_nc(g, topo.n_nodes + 8))
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((gn, g.window_group_incidents_buffer(), g.window_group_tracks_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for gn, (ip, cp, np_), (tp, ep, ecp) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                inc = _d2h(hip, ip, cnt, engine.INCIDENT_DTYPE) if cnt else np.zeros(0, engine.INCIDENT_DTYPE)
                want, wended = ref.step(gn, _d2h(hip, np_, len(gn), np.uint32), inc)
                got = _d2h(hip, tp, cnt, engine.TRACK_DTYPE) if cnt else np.zeros(0, engine.TRACK_DTYPE)
                assert got.tobytes() == want.tobytes()
                n_ended = int(_d2h(hip, ecp, 1, np.uint64)[0])
                assert n_ended == len(wended)
                assert n_ended == 0 or _d2h(hip, ep, n_ended, engine.TRACK_ENTRY_DTYPE).tobytes() == wended.tobytes()
                seen += cnt
            pending = []
    assert seen > 0 and g.group_track_entries().tobytes() == ref.entries().tobytes() and g.group_track_stats().windows == 9


# ---- 5. boundaries ---------------------------------------------------------------------------------------------------------------------
MG = 3000                                                             # max_groups: KNOWN ids on either side of it, and labels above both


@pytest.fixture(scope="module")
def big():
    """4200 pods, max_groups 3000: workload 5 = pods 0, 1; workloads 0 .. 2 = pods 2, 3, 4; pod 9 = workload 2999 (the last group
    key); everything else ungrouped (pod 10's key is max_groups + 10).  Every group edge red"""
    topo, g, mk, mg = _pods(4200, max_groups=MG, labels=16)
    g.group_assign([0, 1, 2, 3, 4, 9], [5, 5, 0, 1, 2, MG - 1])
    g.set_group_nodes(); g.set_group_incidents(**ALL)
    return topo, g, mk


def _fresh(big, quiet=2):
    topo, g, mk = big
    g.set_group_tracks(quiet_windows=quiet)                           # re-enabling starts an empty state
    return topo, g, GroupTrackRef(quiet, 0, ncap=_nc(g, MG))


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_row_counts_around_a_round_of_256_rows(big, n):
    """n workload rows in pairs and one triple, held two windows, then shifted by one row: the heads on either side of 256"""
    topo, g, ref = _fresh(big)
    ids = 50 + np.arange(n)
    src = ids[:-1][::2] if n % 2 == 0 else np.concatenate([ids[:-1][::2], [ids[-2]]])
    pairs = list(zip(src.tolist(), (src + 1).tolist()))
    for w in range(2):
        got, ended, inc = _window(topo, g, ref, pairs)
        assert len(g.window_group_nodes()) == n and len(got) == n // 2 and (got["windows"] == w + 1).all()
        assert ((got["kept_nodes"] if w else got["joined_nodes"]) == inc["nodes"]).all()
    got, ended, _ = _window(topo, g, ref, [(a + 1, b + 1) for a, b in pairs])   # every pair now bridges two tracks
    assert (got["flags"] & MERGED).any() and (got["kept_nodes"] >= 1).all()


def test_one_chain_of_4097_workloads_held_two_windows(big):
    """every workload row folds into one incident word, across the 2048 rows of a folding workgroup"""
    topo, g, ref = _fresh(big)
    n = 4097
    pairs = _chain(np.random.default_rng(4097).permutation(n) + 20)
    got, _, _ = _window(topo, g, ref, pairs)
    assert (got[0]["track"], got[0]["joined_nodes"], got[0]["flags"]) == (0, n, NEW)
    got, _, _ = _window(topo, g, ref, pairs)
    assert (got[0]["track"], got[0]["kept_nodes"], got[0]["joined_nodes"], got[0]["windows"], got[0]["flags"]) == (0, n, 0, 2, 0)


def test_700_two_workload_incidents_in_alternating_halves():
    """max_edges 1024: the workload rows' capacity is 2048, ONE workgroup of k19_look / k13_fold.  The halves alternate (the
    compaction, the opened tracks' ranks and the ended list); then all 700 at once, more distinct incidents than the 512 slots of the
    workgroup's LDS table: at least 188 fold cand, joined, kept and moved into device memory directly; then the pairs shifted by one
    pod, so that every incident bridges two tracks — one workload kept, one moved.  Pods 0 .. 699 are workloads, the rest ungrouped"""
    topo, g, ref = _tracked(1400, quiet=2, grouped=700, max_edges=1024)
    assert 2 * g.max_edges == 2048                                    # one folding workgroup (tests/test_group_track_host.py: fold_wgs)
    halves = [[(2 * k, 2 * k + 1) for k in range(700) if k % 2 == h] for h in (0, 1)]
    for w in range(4):
        got, ended, _ = _window(topo, g, ref, halves[w % 2])
        assert len(got) == 350 and len(ended) == (350 if w else 0)
        assert got["track"].tolist() == list(range(350 * (w % 2), 350 * (w % 2) + 350)) and (got["windows"] == w // 2 + 1).all()
    assert len(g.group_track_entries()) == 700 and g.group_track_stats().opened == 700
    got, ended, _ = _window(topo, g, ref, halves[0] + halves[1])
    assert len(got) == 700 and len(ended) == 0 and (got["flags"] == 0).all() and (got["kept_nodes"] == 2).all()
    got, ended, _ = _window(topo, g, ref, [(2 * k + 1, 2 * k + 2) for k in range(699)])
    assert len(got) == 699 and (got["kept_nodes"] == 1).all() and (got["moved_nodes"] == 1).all() and (got["flags"] & MERGED != 0).all()
    assert (got["flags"] & SPLIT != 0).any()                          # (the halves' ids interleave: two pairs can name one oldest track)


def test_keys_on_both_sides_of_max_groups_and_of_the_anchor_bound(big):
    """a group (the last group key), an ungrouped pod (the first key above max_groups), a label (the last anchor key) and an outbound
    IP (the first key above the anchors) in incidents of their own, held two windows: the first three are kept, the outbound IP
    never is"""
    topo, g, ref = _fresh(big)
    pod = _events(topo, [9, 10, 0], topo.pod_ips[[1000, 1001, 1002]])  # workload 2999, pod 10 and workload 5 each call a pod
    ext = _events(topo, [2000, 2001, 2002], EXT + np.arange(3, dtype=np.uint32), label=[16, 0, 1])   # labels 15 and 0, one raw address
    for w in range(2):
        g.ingest_bulk(np.concatenate([pod, ext])); g.flush_window()
        got, _ = _check(g, ref)
        gn, ninc = g.window_group_nodes(), g.window_group_node_incident()
        refs = gn["ref"].tolist()
        assert {0, 1, 2, 3} == set((gn["ref"] >> 30).tolist()) and len(got) == 6 and (ninc != engine.NO_INCIDENT).all()
        for r in (G(MG - 1), G(5), 10, LABEL | 15, LABEL | 0):
            assert r in refs, r
        anchors = np.bincount(ninc[(gn["ref"] >> 30) != 2], minlength=6)
        assert ((got["kept_nodes"] if w else got["joined_nodes"]) == anchors).all() and (got["moved_nodes"] == 0).all()
        ob = int(ninc[(gn["ref"] >> 30) == 2][0])                     # the incident of pod 2001 and its raw address
        assert g.window_group_incidents()["nodes"][ob] == 2 and anchors[ob] == 1
        assert (got["flags"] == (0 if w else NEW)).all()


def test_a_window_of_no_incident_and_a_window_of_no_group_edge(big):
    topo, g, ref = _fresh(big, quiet=1)
    c = _chain([20, 21, 22])
    _window(topo, g, ref, c)
    got, ended, _ = _window(topo, g, ref, [])                         # no group edge at all
    assert len(got) == 0 and ended["track"].tolist() == [0] and len(g.window_groups()) == 0
    g.set_group_incidents(by="score", min_value=INF); g.set_group_tracks(quiet_windows=1)   # (the switch takes the stage with it)
    try:
        ref = GroupTrackRef(1, 0, ncap=_nc(g, MG))
        got, ended, _ = _window(topo, g, ref, c)                      # group edges, none of them red: no incident
        assert len(got) == 0 and len(ended) == 0 and len(g.window_groups()) == 2 and len(g.group_track_entries()) == 0
    finally:
        g.set_group_incidents(**ALL)


# ---- 6. track behaviour ----------------------------------------------------------------------------------------------------------------
def test_64_disjoint_chains_held_three_windows_then_a_new_one():
    n = sum(h + 1 for h in range(1, 65)) + 3
    topo, g, ref = _tracked(n, grouped=n // 2)
    perm = np.random.default_rng(64).permutation(n - 3)
    pairs, at = [], 0
    for h in range(1, 65):
        pairs += _chain(perm[at:at + h + 1]); at += h + 1
    for w in range(3):
        got, ended, inc = _window(topo, g, ref, pairs)
        assert sorted(got["track"].tolist()) == list(range(64)) and (got["windows"] == w + 1).all() and len(ended) == 0
        assert (got["flags"] == (NEW if w == 0 else 0)).all() and (got["parent"] == NO).all()
        assert ((got["joined_nodes"] if w == 0 else got["kept_nodes"]) == inc["nodes"]).all() and (got["moved_nodes"] == 0).all()
    got, ended, inc = _window(topo, g, ref, pairs + _chain([n - 3, n - 2, n - 1]))
    assert sorted(got["track"].tolist()) == list(range(65)) and int((got["flags"] == NEW).sum()) == 1
    assert g.group_track_stats().opened == 65 and g.group_track_stats().live == 65


def test_two_chains_bridged_merge_into_the_older():
    topo, g, ref = _tracked(16, grouped=5)
    a, b = _chain([1, 2, 3]), _chain([9, 8, 7, 6])
    got, _, _ = _window(topo, g, ref, a + b)
    assert got["track"].tolist() == [0, 1]
    got, ended, _ = _window(topo, g, ref, a + b + [(3, 9)])
    assert len(got) == 1 and (got[0]["track"], got[0]["kept_nodes"], got[0]["moved_nodes"], got[0]["flags"]) == (0, 3, 4, MERGED)
    assert ended["track"].tolist() == [1] and ended["windows"].tolist() == [1]
    got, ended, _ = _window(topo, g, ref, a + b + [(3, 9)])
    assert (got[0]["track"], got[0]["kept_nodes"], got[0]["moved_nodes"], got[0]["flags"], got[0]["windows"]) == (0, 7, 0, 0, 3) and len(ended) == 0


@pytest.mark.parametrize("cut", [4, 5])
def test_a_chain_cut_in_two_splits(cut):
    """workloads 1..10 cut into 1..cut and the rest: 4 / 6 continues in the later, larger piece (by kept), 5 / 5 in the first (the tie)"""
    topo, g, ref = _tracked(16, grouped=12)
    _window(topo, g, ref, _chain(range(1, 11)))
    got, ended, _ = _window(topo, g, ref, _chain(range(1, cut + 1)) + _chain(range(cut + 1, 11)))
    assert len(ended) == 0
    if cut == 4:
        assert got["track"].tolist() == [1, 0] and got["flags"].tolist() == [NEW | SPLIT, 0] and got["kept_nodes"].tolist() == [4, 6]
        assert got["parent"].tolist() == [0, NO]
    else:
        assert got["track"].tolist() == [0, 1] and got["flags"].tolist() == [0, NEW | SPLIT] and got["kept_nodes"].tolist() == [5, 5]
        assert got["parent"].tolist() == [NO, 0]


@pytest.mark.parametrize("quiet", [1, 2])
def test_a_flap_keeps_its_id_and_one_window_more_does_not(quiet):
    topo, g, ref = _tracked(16, quiet=quiet, grouped=3)
    c = _chain([2, 3, 4])
    _window(topo, g, ref, c)
    listed = 0
    for _ in range(quiet):
        listed += len(_window(topo, g, ref, [])[1])
        assert g.group_track_entries()["track"].tolist() == [0]
    got, ended, _ = _window(topo, g, ref, c)
    assert (got[0]["track"], got[0]["windows"], got[0]["flags"]) == (0, 2, 0) and listed + len(ended) == 1
    for k in range(quiet + 1):
        assert len(_window(topo, g, ref, [])[1]) == (1 if k == 0 else 0)
    assert len(g.group_track_entries()) == 0                          # the old entry is gone
    got, _, _ = _window(topo, g, ref, c)
    assert (got[0]["track"], got[0]["parent"], got[0]["windows"], got[0]["flags"]) == (1, NO, 1, NEW)
    assert g.group_track_entries()["track"].tolist() == [1]


def test_max_tracks_cuts_the_table():
    n = sum(h + 1 for h in range(1, 65))
    topo, g, ref = _tracked(n, max_tracks=8, grouped=n // 2)
    perm = np.random.default_rng(65).permutation(n)
    pairs, at = [], 0
    for h in range(1, 65):
        pairs += _chain(perm[at:at + h + 1]); at += h + 1
    got, _, _ = _window(topo, g, ref, pairs)
    assert sorted(got["track"].tolist()) == list(range(64)) and g.group_track_entries()["track"].tolist() == list(range(8))
    assert g.group_track_stats().dropped_cap == 56
    got, _, _ = _window(topo, g, ref, pairs)
    assert sorted(got["track"].tolist()) == list(range(8)) + list(range(64, 120)) and g.group_track_stats().dropped_cap == 112
    assert int((got["flags"] == NEW).sum()) == 56 and int((got["flags"] == 0).sum()) == 8


# ---- 7. the close paths ----------------------------------------------------------------------------------------------------------------
def _churn_engine(churn, quiet=2, **kw):
    topo, labels, wins = churn
    one, _, mk = _grouped(topo, labels, "blocks")
    _feed(one, wins[0]); one.flush_window()
    thr = quantile_threshold(one.window_groups()["score_max"], 0.9)
    g, _, _ = _grouped(topo, labels, "blocks", **kw)
    g.set_group_nodes(); g.set_group_incidents(min_value=thr); g.set_group_tracks(quiet_windows=quiet)
    return g, GroupTrackRef(quiet, 0, ncap=_nc(g, mk)), thr


def test_every_close_path_gives_the_same_rows(churn):
    topo, labels, wins = churn
    g, ref, _ = _churn_engine(churn)
    reads = (g.window_group_incident_tracks, g.window_group_tracks_ended)
    for i, w in enumerate(wins[:7]):
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in reads:
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            assert _rc(g.set_group_tracks) == engine.SG_ESTATE and _rc(g.set_group_tracks, None) == engine.SG_ESTATE
            assert _err(g.window_group_tracks_ended)[1] == "sg_window_group_tracks_ended while a flush is open"
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
        _check(g, ref)
    assert g.group_track_stats().opened > 0


@pytest.mark.parametrize("in_flight", [1, 3])
def test_window_run_in_flight(churn, in_flight):
    """each slot's rows against its own window, the state updated in window order; read only after a round of slots was enqueued"""
    import torch
    topo, labels, wins = churn
    g, ref, thr = _churn_engine(churn, windows_in_flight=in_flight)
    one, _, _ = _grouped(topo, labels, "blocks")
    one.set_group_nodes()
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    torch.cuda.synchronize()
    pending = []
    for i, w in enumerate(wins[:6]):
        _feed(one, w); one.flush_window()
        gn = one.window_group_nodes()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((gn, g.window_group_incidents_buffer(), g.window_group_tracks_buffer()))
        if len(pending) == in_flight:
            torch.cuda.synchronize()
            for gn, (ip, cp, np_), (tp, ep, ecp) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                inc = _d2h(hip, ip, cnt, engine.INCIDENT_DTYPE) if cnt else np.zeros(0, engine.INCIDENT_DTYPE)
                want, wended = ref.step(gn, _d2h(hip, np_, len(gn), np.uint32), inc)
                got = _d2h(hip, tp, cnt, engine.TRACK_DTYPE) if cnt else np.zeros(0, engine.TRACK_DTYPE)
                assert got.tobytes() == want.tobytes()
                n_ended = int(_d2h(hip, ecp, 1, np.uint64)[0])
                assert n_ended == len(wended)
                assert n_ended == 0 or _d2h(hip, ep, n_ended, engine.TRACK_ENTRY_DTYPE).tobytes() == wended.tobytes()
            pending = []
    assert g.group_track_entries().tobytes() == ref.entries().tobytes() and g.group_track_stats().windows == 6


# ---- 8. the twin -----------------------------------------------------------------------------------------------------------------------
def test_a_twin_without_it_is_unchanged(churn):
    """every other output of an engine with the stage against a twin without it (K8 - K13 and K14 - K18 on in both); the twin's
    reads are SG_ESTATE"""
    topo, labels, wins = churn
    (g, _, mk), (twin, _, _) = _grouped(topo, labels, "blocks"), _grouped(topo, labels, "blocks")
    for x in (g, twin):
        x.set_trend(**TREND); x.set_nodes(); x.set_rank(iters=2); x.set_incidents(min_value=0.5); x.set_tracks(quiet_windows=1)
        x.set_group_trend(**TREND); x.set_group_vanished(silent_windows=1, min_seen=1)
        x.set_group_nodes(); x.set_group_node_trend(shift=3, warmup=2, ttl=2); x.set_group_rank(iters=3)
        x.set_group_incidents(min_value=0.5)
    g.set_group_tracks(quiet_windows=1)
    ref = GroupTrackRef(1, 0, ncap=_nc(g, mk))
    for w in wins[:6]:
        _feed(g, w); _feed(twin, w)
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        for name in ("window_trend", "window_nodes", "window_rank", "window_incidents", "window_node_incident", "window_incident_tracks",
                     "window_tracks_ended", "track_entries", "window_groups", "window_row_group", "window_group_trend",
                     "window_group_vanished", "window_group_nodes", "window_group_node_trend", "window_group_rank", "window_group_incidents",
                     "window_group_node_incident"):
            assert getattr(g, name)().tobytes() == getattr(twin, name)().tobytes(), name
        _check(g, ref)
    assert g.trend_entries().tobytes() == twin.trend_entries().tobytes()
    assert g.group_trend_entries().tobytes() == twin.group_trend_entries().tobytes()
    assert g.group_node_trend_entries().tobytes() == twin.group_node_trend_entries().tobytes()
    for call in (twin.window_group_incident_tracks, twin.window_group_tracks_ended, twin.window_group_tracks_buffer, twin.group_track_entries,
                 twin.group_track_stats):
        assert _rc(call) == engine.SG_ESTATE


# ---- 9. lifecycle and error codes --------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    mk = topo.n_nodes + 8
    calls = (g.window_group_incident_tracks, g.window_group_tracks_ended, g.window_group_tracks_buffer, g.group_track_entries,
             g.group_track_stats)
    ON = dict(min_value=-INF)

    def all_off():
        for c in calls:
            assert _rc(c) == engine.SG_ESTATE
    assert _rc(g.set_group_tracks) == engine.SG_ESTATE and _rc(g.set_group_tracks, None) == engine.SG_ESTATE   # the groups are off
    all_off()
    g.set_groups(); g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7)
    assert _rc(g.set_group_tracks) == engine.SG_ESTATE
    g.set_group_nodes()
    assert _err(g.set_group_tracks) == (engine.SG_ESTATE, "sg_set_group_tracks: the workload incidents are off (sg_set_group_incidents)")
    all_off()
    g.set_group_incidents(**ON)
    all_off()                                                          # off by default
    assert _err(g.group_track_entries) == (engine.SG_ESTATE, "sg_group_track_entries: workload tracking is off (sg_set_group_tracks)")
    assert _err(g.set_group_tracks, reserved=1) == (engine.SG_EINVAL, "sg_set_group_tracks: bad parameters")
    for bad in (dict(quiet_windows=16), dict(struct_size=12), dict(struct_size=20), dict(reserved=1)):
        assert _rc(g.set_group_tracks, **bad) == engine.SG_EINVAL
    _feed(g, wins[0]); g.flush_window()
    g.set_group_tracks(quiet_windows=1)
    assert _err(g.window_group_incident_tracks) == (engine.SG_ESTATE, "sg_window_group_incident_tracks: the last read window was closed "
                                                    "while workload tracking was off")   # the read window was closed before it was on
    assert _rc(g.window_group_tracks_ended) == engine.SG_ESTATE and _rc(g.window_group_tracks_buffer) == engine.SG_ESTATE
    assert len(g.group_track_entries()) == 0 and g.group_track_stats().windows == 0
    ref = GroupTrackRef(1, 0, ncap=_nc(g, mk))
    for w in wins[1:3]:
        _feed(g, w); g.flush_window()
        _check(g, ref)
    assert g.group_track_stats().opened > 0
    g.set_group_tracks(quiet_windows=0, max_tracks=5)                  # re-enabling restarts at w = 0, id 0
    assert len(g.group_track_entries()) == 0 and g.group_track_stats().opened == 0
    assert _rc(g.window_group_incident_tracks) == engine.SG_ESTATE
    ref = GroupTrackRef(0, 5)
    _feed(g, wins[3]); g.flush_window()
    got, _ = _check(g, ref)
    assert got["track"].tolist() == list(range(len(got))) and (got["first_window"] == 0).all()
    # K13 beside it: neither disturbs the other
    g.set_nodes(); g.set_incidents(**ON); g.set_tracks(quiet_windows=0)
    _feed(g, wins[4]); g.flush_window()
    _check(g, ref)
    assert g.track_stats().windows == 1 and g.group_track_stats().windows == 2
    g.set_tracks(None); g.set_incidents(None)
    _feed(g, wins[5]); g.flush_window()
    _check(g, ref)
    g.set_incidents(**ON); g.set_tracks()
    g.set_group_tracks(None)
    all_off()
    _feed(g, wins[6]); g.flush_window()
    assert g.track_stats().windows == 1 and len(g.window_incident_tracks()) == len(g.window_incidents())
    g.set_nodes(False)
    # every sg_set_group_incidents call, on or off, switches the stage off
    g.set_group_tracks()
    g.set_group_incidents(**ON)
    all_off()
    g.set_group_tracks()
    g.set_group_incidents(None)
    all_off()
    assert _rc(g.set_group_tracks) == engine.SG_ESTATE
    g.set_group_incidents(**ON); g.set_group_tracks()
    g.set_group_nodes(False)                                          # the workload rows off take the incidents and the tracks with them
    all_off()
    g.set_group_nodes(); g.set_group_incidents(**ON); g.set_group_tracks()
    g.set_groups()                                                    # any sg_set_groups call frees it
    all_off()
    assert _rc(g.set_group_tracks) == engine.SG_ESTATE
    g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7)
    g.set_group_nodes(); g.set_group_incidents(**ON)
    _feed(g, wins[7]); g.flush_window()
    assert len(g.window_group_incidents()) > 0 and _rc(g.window_group_incident_tracks) == engine.SG_ESTATE
    g.set_group_tracks()
    ref = GroupTrackRef(2, 0, ncap=_nc(g, mk))
    _feed(g, wins[8]); g.flush_window()
    got, _ = _check(g, ref)
    assert len(got) > 0 and (got["flags"] == NEW).all() and (got["first_window"] == 0).all()
