"""K13, the tracks (sg_set_tracks / sg_window_incident_tracks / sg_window_tracks_ended / sg_window_tracks_buffer / sg_track_entries /
sg_track_stats_get): the rows, the ended list and the table of every window against the pure-Python reference tests/track_ref.py fed
with the engine's own node rows, incident rows and incident per node row of the same window — byte for byte, every field is an
integer — on every close path, an engine with it against a twin without it, and constructed windows whose answers are known."""
import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import _d2h, _engine, _feed, _hip, _incident_close as _close, _incident_pods_engine as _pods_engine, _ncap, _rc
from tests.incident_ref import quantile_threshold
from tests.traces import churn  # noqa: F401  (the fixtures)
from tests.track_ref import TrackRef

pytestmark = pytest.mark.gpu

INF = float("inf")
NO = engine.NO_TRACK
NEW, SPLIT, MERGED = engine.TRACK_NEW, engine.TRACK_SPLIT, engine.TRACK_MERGED
TREND = dict(shift=3, warmup=2, ttl=4)


def _check(g, ref):
    """the last read window's track rows, ended list and the table after it against the reference's step over the same window"""
    nodes, inc, ninc = g.window_nodes(), g.window_incidents(), g.window_node_incident()
    want, wended = ref.step(nodes, ninc, inc)
    got, ended = g.window_incident_tracks(), g.window_tracks_ended()
    assert len(got) == len(want) == len(inc)
    assert got.tobytes() == want.tobytes(), (ref.w - 1, got.tolist(), want.tolist())
    assert ended.tobytes() == wended.tobytes(), (ref.w - 1, ended.tolist(), wended.tolist())
    assert g.track_entries().tobytes() == ref.entries().tobytes(), ref.w - 1
    s = g.track_stats()
    assert dict(windows=s.windows, live=s.live, opened=s.opened, dropped_cap=s.dropped_cap) == ref.stats()
    return got, ended


# ---- the churn ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quiet,by,ranked", [(0, "score", False), (2, "score", False), (2, "lat_dev", True)])
def test_every_window_of_the_churn_is_exact(churn, quiet, by, ranked):
    topo, labels, wins = churn
    twin, g = _engine(topo, labels), _engine(topo, labels)
    for x in (twin, g):
        x.set_nodes()
        if by != "score":
            x.set_trend(**TREND)
        if ranked:
            x.set_rank(iters=3)
    if by == "score":                                                 # the threshold: fixed, the 0.9 quantile of a twin's window
        _feed(twin, wins[0])
        thr = quantile_threshold(twin.flush_window()["score"], 0.9)
    else:
        for w in wins[:4]:
            _feed(twin, w); twin.flush_window()
        thr = quantile_threshold(twin.window_trend()[by], 0.9)
    g.set_incidents(by=by, min_value=thr)
    g.set_tracks(quiet_windows=quiet)
    ref = TrackRef(quiet, 0, ncap=_ncap(g))
    flags, continued = 0, 0
    for w in wins:
        _feed(g, w); g.flush_window()
        got, ended = _check(g, ref)
        flags |= int(np.bitwise_or.reduce(got["flags"])) if len(got) else 0
        continued += int(((got["flags"] & NEW) == 0).sum())
    assert flags & NEW and continued > 0 and g.track_stats().opened > 0


def test_a_twin_without_it_is_unchanged(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(**TREND); x.set_rank(iters=3)
    _feed(twin, wins[0]); _feed(g, wins[0])
    thr = quantile_threshold(twin.flush_window()["score"], 0.9)
    g.flush_window()
    for x in (g, twin):
        x.set_incidents(min_value=thr)
    g.set_tracks(quiet_windows=1)
    ref = TrackRef(1, 0, ncap=_ncap(g))
    assert _rc(twin.window_incident_tracks) == engine.SG_ESTATE
    for w in wins[1:7]:
        _feed(g, w); _feed(twin, w)
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        assert g.window_nodes().tobytes() == twin.window_nodes().tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_rank().tobytes() == twin.window_rank().tobytes()
        assert g.window_incidents().tobytes() == twin.window_incidents().tobytes()
        assert g.window_node_incident().tobytes() == twin.window_node_incident().tobytes()
        _check(g, ref)
    assert g.trend_entries().tobytes() == twin.trend_entries().tobytes()


# ---- constructed windows: pod-to-pod events only and min_value = -inf, so a window's incidents are exactly the components fed -------
def _tracked(n_pods, quiet=2, max_tracks=0):
    topo, g = _pods_engine(n_pods)
    g.set_tracks(quiet_windows=quiet, max_tracks=max_tracks)
    return topo, g, TrackRef(quiet, max_tracks, ncap=_ncap(g))


def _window(topo, g, ref, pairs):
    """close a window of one request per (src pod, dst pod) pair (none: an empty window); (track rows, ended, incident rows, incident per node)"""
    if len(pairs):
        src, dst = zip(*pairs)
        _, _, inc, ninc = _close(topo, g, src, dst)
    else:
        assert len(g.flush_window()) == 0
        inc, ninc = g.window_incidents(), g.window_node_incident()
        assert len(inc) == 0 and len(ninc) == 0
    got, ended = _check(g, ref)
    return got, ended, inc, ninc


def _chain(ids):
    ids = [int(x) for x in ids]
    return list(zip(ids[:-1], ids[1:]))


def test_64_disjoint_chains_held_three_windows_then_a_new_one():
    n = sum(h + 1 for h in range(1, 65)) + 3
    topo, g, ref = _tracked(n)
    perm = np.random.default_rng(64).permutation(n - 3)
    pairs, at = [], 0
    for h in range(1, 65):
        pairs += _chain(perm[at:at + h + 1]); at += h + 1
    for w in range(3):
        got, ended, inc, _ = _window(topo, g, ref, pairs)
        assert got["track"].tolist() == list(range(64)) and (got["windows"] == w + 1).all() and len(ended) == 0
        assert (got["flags"] == (NEW if w == 0 else 0)).all() and (got["parent"] == NO).all()
        assert ((got["joined_nodes"] if w == 0 else got["kept_nodes"]) == inc["nodes"]).all() and (got["moved_nodes"] == 0).all()
    got, ended, inc, _ = _window(topo, g, ref, pairs + _chain([n - 3, n - 2, n - 1]))
    assert sorted(got["track"].tolist()) == list(range(65)) and got["track"][inc["first_node"] == n - 3].tolist() == [64]
    assert g.track_stats().opened == 65 and g.track_stats().live == 65


def test_two_chains_bridged_merge_into_the_older():
    topo, g, ref = _tracked(16)
    a, b = _chain([1, 2, 3]), _chain([9, 8, 7, 6])
    got, _, _, _ = _window(topo, g, ref, a + b)
    assert got["track"].tolist() == [0, 1]
    got, ended, _, _ = _window(topo, g, ref, a + b + [(3, 9)])
    assert len(got) == 1 and (got[0]["track"], got[0]["kept_nodes"], got[0]["moved_nodes"], got[0]["flags"]) == (0, 3, 4, MERGED)
    assert ended["track"].tolist() == [1] and ended["windows"].tolist() == [1]
    got, ended, _, _ = _window(topo, g, ref, a + b + [(3, 9)])
    assert (got[0]["track"], got[0]["kept_nodes"], got[0]["moved_nodes"], got[0]["flags"], got[0]["windows"]) == (0, 7, 0, 0, 3) and len(ended) == 0


@pytest.mark.parametrize("cut", [4, 5])
def test_a_chain_cut_in_two_splits(cut):
    """pods 1..10 cut into 1..cut and the rest: 4 / 6 continues in the later, larger piece (by kept), 5 / 5 in the first (the tie)"""
    topo, g, ref = _tracked(16)
    _window(topo, g, ref, _chain(range(1, 11)))
    got, ended, _, _ = _window(topo, g, ref, _chain(range(1, cut + 1)) + _chain(range(cut + 1, 11)))
    assert len(ended) == 0
    if cut == 4:
        assert got["track"].tolist() == [1, 0] and got["flags"].tolist() == [NEW | SPLIT, 0] and got["kept_nodes"].tolist() == [4, 6]
        assert got["parent"].tolist() == [0, NO]
    else:
        assert got["track"].tolist() == [0, 1] and got["flags"].tolist() == [0, NEW | SPLIT] and got["kept_nodes"].tolist() == [5, 5]
        assert got["parent"].tolist() == [NO, 0]


@pytest.mark.parametrize("quiet", [1, 2])
def test_a_flap_keeps_its_id_and_one_window_more_does_not(quiet):
    topo, g, ref = _tracked(16, quiet=quiet)
    c = _chain([2, 3, 4])
    _window(topo, g, ref, c)
    listed = 0
    for _ in range(quiet):
        listed += len(_window(topo, g, ref, [])[1])
        assert g.track_entries()["track"].tolist() == [0]
    got, ended, _, _ = _window(topo, g, ref, c)
    assert (got[0]["track"], got[0]["windows"], got[0]["flags"]) == (0, 2, 0) and listed + len(ended) == 1
    for k in range(quiet + 1):
        assert len(_window(topo, g, ref, [])[1]) == (1 if k == 0 else 0)
    assert len(g.track_entries()) == 0                                # the old entry is gone
    got, _, _, _ = _window(topo, g, ref, c)
    assert (got[0]["track"], got[0]["parent"], got[0]["windows"], got[0]["flags"]) == (1, NO, 1, NEW)
    assert g.track_entries()["track"].tolist() == [1]


def test_700_two_pod_incidents_in_alternating_halves():
    """more than one workgroup of incidents and of table entries: the compaction, the opened tracks' ranks and the ended list cross
    workgroup boundaries (more incidents than a folding workgroup's table has slots: the test below)"""
    topo, g, ref = _tracked(1400, quiet=2)
    halves = [[(2 * k, 2 * k + 1) for k in range(700) if k % 2 == h] for h in (0, 1)]
    for w in range(4):
        got, ended, _, _ = _window(topo, g, ref, halves[w % 2])
        assert len(got) == 350 and len(ended) == (350 if w else 0)
        assert got["track"].tolist() == list(range(350 * (w % 2), 350 * (w % 2) + 350)) and (got["windows"] == w // 2 + 1).all()
    assert len(g.track_entries()) == 700 and g.track_stats().opened == 700
    got, ended, _, _ = _window(topo, g, ref, halves[0] + halves[1])
    assert len(got) == 700 and len(ended) == 0 and (got["flags"] == 0).all()


def test_more_incidents_than_table_slots_in_one_workgroup():
    """700 two-pod incidents at once in an engine whose node rows all go through ONE workgroup of k13_look / k13_fold (the plan gives
    a folding workgroup 2 048 node rows): more distinct incidents than the 512 slots of its LDS table, so at least 188 of them find no
    slot and fold cand, joined, kept and moved into device memory directly.  Window 0: every node joins; window 1: every node is
    kept; window 2: the pairs shifted by one pod, so that every incident bridges two tracks — one node kept, one moved."""
    topo, g, ref = _tracked(1400, quiet=0)
    assert 1400 <= _ncap(g) <= 2048                                   # one folding workgroup (tests/test_track_host.py: fold_wgs)
    pairs = [(2 * k, 2 * k + 1) for k in range(700)]
    got, _, _, _ = _window(topo, g, ref, pairs)
    assert got["track"].tolist() == list(range(700)) and (got["joined_nodes"] == 2).all() and (got["flags"] == NEW).all()
    got, ended, _, _ = _window(topo, g, ref, pairs)
    assert got["track"].tolist() == list(range(700)) and (got["kept_nodes"] == 2).all() and (got["flags"] == 0).all() and len(ended) == 0
    got, ended, _, _ = _window(topo, g, ref, [(2 * k + 1, 2 * k + 2) for k in range(699)])
    assert got["track"].tolist() == list(range(699)) and (got["kept_nodes"] == 1).all() and (got["moved_nodes"] == 1).all()
    assert (got["flags"] == MERGED).all() and ended["track"].tolist() == [699]


def test_one_chain_of_4097_pods_held_two_windows():
    """every node row folds into one incident word"""
    n = 4097
    topo, g, ref = _tracked(n)
    pairs = _chain(np.random.default_rng(4097).permutation(n))
    got, _, _, _ = _window(topo, g, ref, pairs)
    assert (got[0]["track"], got[0]["joined_nodes"], got[0]["flags"]) == (0, n, NEW)
    got, _, _, _ = _window(topo, g, ref, pairs)
    assert (got[0]["track"], got[0]["kept_nodes"], got[0]["joined_nodes"], got[0]["windows"], got[0]["flags"]) == (0, n, 0, 2, 0)


def test_max_tracks_cuts_the_table():
    n = sum(h + 1 for h in range(1, 65))
    topo, g, ref = _tracked(n, max_tracks=8)
    perm = np.random.default_rng(65).permutation(n)
    pairs, at = [], 0
    for h in range(1, 65):
        pairs += _chain(perm[at:at + h + 1]); at += h + 1
    got, _, _, _ = _window(topo, g, ref, pairs)
    assert got["track"].tolist() == list(range(64)) and g.track_entries()["track"].tolist() == list(range(8))
    assert g.track_stats().dropped_cap == 56
    got, _, _, _ = _window(topo, g, ref, pairs)
    assert got["track"].tolist() == list(range(8)) + list(range(64, 120)) and g.track_stats().dropped_cap == 112
    assert (got["flags"][8:] == NEW).all() and (got["flags"][:8] == 0).all()


def _pair_sequence(seed, windows=12, pods=300):
    """pod pairs that drift: some die and some are born per window, now and then most die or the window is empty"""
    rng = np.random.default_rng(300 + seed)
    alive, out = set(), []
    for w in range(windows):
        if rng.random() < 0.2:
            alive = {p for p in alive if rng.random() < 0.3}
        alive = {p for p in alive if rng.random() < 0.8}
        for _ in range(int(rng.integers(5, 40))):
            a, b = (int(x) for x in rng.integers(0, pods, 2))
            if a != b and (b, a) not in alive:
                alive.add((a, b))
        out.append(sorted(alive) if w % 5 != 3 else [])
    return out


@pytest.mark.parametrize("seed", range(4))
def test_a_random_sequence_of_pod_pairs(seed):
    topo, g, ref = _tracked(300, quiet=seed % 3)
    flags = 0
    for pairs in _pair_sequence(seed):
        got, _, _, _ = _window(topo, g, ref, pairs)
        flags |= int(np.bitwise_or.reduce(got["flags"])) if len(got) else 0
    assert flags == NEW | SPLIT | MERGED                              # (tests/test_track_host.py's reference meets all three on these)


# ---- the close paths -----------------------------------------------------------------------------------------------------------------
def _churn_engine(churn, quiet=2, **kw):
    topo, labels, wins = churn
    one = _engine(topo, labels)
    _feed(one, wins[0])
    thr = quantile_threshold(one.flush_window()["score"], 0.9)
    g = _engine(topo, labels, **kw)
    g.set_nodes(); g.set_incidents(min_value=thr); g.set_tracks(quiet_windows=quiet)
    return g, TrackRef(quiet, 0, ncap=_ncap(g)), thr


def test_begin_end_view_and_top(churn):
    topo, labels, wins = churn
    g, ref, _ = _churn_engine(churn)
    for i, w in enumerate(wins[:8]):
        _feed(g, w)
        if i % 4 == 0:
            g.flush_begin()
            assert _rc(g.window_incident_tracks) == engine.SG_ESTATE    # a flush is open
            assert _rc(g.window_tracks_ended) == engine.SG_ESTATE
            assert _rc(g.set_tracks) == engine.SG_ESTATE and _rc(g.set_tracks, None) == engine.SG_ESTATE
            g.flush_end()
        elif i % 4 == 1:
            g.flush_window_view()
        elif i % 4 == 2:
            g.flush_begin(); g.flush_end_view()
        else:
            g.flush_window_top(3)
        _check(g, ref)


@pytest.mark.parametrize("in_flight", [1, 3])
def test_window_run_in_flight(churn, in_flight):
    """sg_window_run with windows in flight: each slot's rows against its own window, the state updated in window order; read only
    after a round of slots was enqueued"""
    import torch
    topo, labels, wins = churn
    g, ref, thr = _churn_engine(churn, windows_in_flight=in_flight)
    one = _engine(topo, labels)
    one.set_nodes()
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending = []
    for i, w in enumerate(wins[:9]):
        _feed(one, w); one.flush_window()
        nodes = one.window_nodes()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((nodes, g.window_incidents_buffer(), g.window_tracks_buffer()))
        if len(pending) == in_flight or i == 8:
            torch.cuda.synchronize()
            for nodes, (ip, cp, np_), (tp, ep, ecp) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                inc = _d2h(hip, ip, cnt, engine.INCIDENT_DTYPE)
                ninc = _d2h(hip, np_, len(nodes), np.uint32)
                want, wended = ref.step(nodes, ninc, inc)
                assert _d2h(hip, tp, cnt, engine.TRACK_DTYPE).tobytes() == want.tobytes()
                n_ended = int(_d2h(hip, ecp, 1, np.uint64)[0])
                assert n_ended == len(wended) and _d2h(hip, ep, n_ended, engine.TRACK_ENTRY_DTYPE).tobytes() == wended.tobytes()
            pending = []
    assert g.track_entries().tobytes() == ref.entries().tobytes() and g.track_stats().windows == 9


def test_window_run_and_read(churn):
    topo, labels, wins = churn
    g, ref, _ = _churn_engine(churn, variant=2)
    for w in wins[:3]:
        _feed(g, w)
        g.window_run()
        g.window_read()
        _check(g, ref)


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_k1_variants(churn, variant):
    topo, labels, wins = churn
    g, ref, _ = _churn_engine(churn, variant=variant)
    for w in wins[:2]:
        _feed(g, w); g.flush_window()
        _check(g, ref)


# ---- lifecycle and error codes ---------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    calls = (g.window_incident_tracks, g.window_tracks_ended, g.window_tracks_buffer, g.track_entries, g.track_stats)
    assert _rc(g.set_tracks) == engine.SG_ESTATE                       # the incidents are off
    g.set_nodes()
    assert _rc(g.set_tracks) == engine.SG_ESTATE
    g.set_incidents(min_value=-INF)
    for c in calls:
        assert _rc(c) == engine.SG_ESTATE                              # off by default
    for bad in (dict(quiet_windows=16), dict(struct_size=12), dict(struct_size=20), dict(reserved=1)):
        assert _rc(g.set_tracks, **bad) == engine.SG_EINVAL
    _feed(g, wins[0]); g.flush_window()
    g.set_tracks(quiet_windows=1)
    assert _rc(g.window_incident_tracks) == engine.SG_ESTATE           # the read window was closed before it was on
    assert len(g.track_entries()) == 0 and g.track_stats().windows == 0
    ref = TrackRef(1, 0, ncap=_ncap(g))
    for w in wins[1:3]:
        _feed(g, w); g.flush_window()
        _check(g, ref)
    assert g.track_stats().opened > 0
    g.set_tracks(quiet_windows=0, max_tracks=5)                        # re-enabling restarts at w = 0, id 0
    assert len(g.track_entries()) == 0 and g.track_stats().opened == 0 and _rc(g.window_incident_tracks) == engine.SG_ESTATE
    ref = TrackRef(0, 5)
    _feed(g, wins[3]); g.flush_window()
    got, _ = _check(g, ref)
    assert got["track"].tolist() == list(range(len(got))) and (got["first_window"] == 0).all()
    g.set_incidents(min_value=-INF)                                    # every sg_set_incidents call switches tracking off
    for c in calls:
        assert _rc(c) == engine.SG_ESTATE
    g.set_tracks()
    g.set_incidents(None)
    assert _rc(g.track_entries) == engine.SG_ESTATE and _rc(g.set_tracks) == engine.SG_ESTATE
    g.set_incidents(min_value=-INF); g.set_tracks()
    g.set_tracks(None)
    assert _rc(g.track_entries) == engine.SG_ESTATE
    g.set_tracks()
    g.set_nodes(False)                                                 # the rollup off takes the incidents and the tracks with it
    for c in calls:
        assert _rc(c) == engine.SG_ESTATE
    g.set_nodes(True); g.set_incidents(min_value=-INF)
    _feed(g, wins[4]); g.flush_window()
    assert len(g.window_incidents()) > 0 and _rc(g.window_incident_tracks) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_nodes, True) == engine.SG_EINVAL
    assert _rc(g.set_incidents) == engine.SG_ESTATE and _rc(g.set_tracks) == engine.SG_ESTATE
