"""K24, the SLO burn rates (sg_set_slo / sg_slo_assign / sg_window_node_slo / sg_window_group_node_slo / sg_window_slo_buffer /
sg_slo_entries / sg_slo_stats_get and the two _top_slo selections): the rows, the state entries and the statistics of both spaces
after every window against tests/slo_ref.py — byte for byte — run on the same engine's own node rows, workload rows and K20
histograms of that window (K20's tables are held to tests/quantile_ref.py by tests/test_gpu_quantiles.py).  Windows are a few
hundred to a few thousand events: the churn of tests/traces.py thinned, and constructed pod-to-pod windows."""
import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import EXT, _d2h, _engine, _events, _feed, _hip, _map, _pods_engine, _rc, _send
from tests.helpers import G
from tests.slo_ref import SloRef, ref_select_slo, slo_values
from tests.traces import churn  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NO = engine.NO_GROUP
BOTH = ("nodes", "group_nodes")
LABEL = 1 << 30
STATS = ("windows", "keys_active", "sides_burning", "keys")
#: the churn's durations fall into bins 1 .. 14 with 7 % above bin 7, and up to 8 % of its requests fail: both kinds burn, neither always
PARAMS = dict(latency_bin=7, latency_target_ppm=950_000, error_target_ppm=990_000, short_windows=2, long_windows=5, min_burn_q10=1024,
              min_requests=10)
READS = dict(nodes=("window_nodes", "window_node_hist", "window_node_slo"),
             group_nodes=("window_group_nodes", "window_group_node_hist", "window_group_node_slo"))


def _stages(g, gmap=None, spaces=BOTH):
    g.set_nodes(); g.set_groups()
    if gmap is not None:
        g.group_assign(np.arange(len(gmap)), gmap)
    g.set_group_nodes()
    g.set_quantiles(spaces)


def _thin(w, step=8):
    return w[::step]


class Slo:
    """the references of one engine's SLO stage and the check of the last read window against them"""

    def __init__(self, g, mk, ml=256, spaces=BOTH, **params):
        self.spaces, self.params = spaces, params
        self.ref = {s: SloRef(s, mk, ml, mk, **params) for s in spaces}   # (max_groups defaults to max_known_nodes)
        g.set_slo(spaces, **params)

    def assign(self, g, space, refs, objectives):
        g.slo_assign(space, refs, objectives)
        self.ref[space].assign(refs, objectives)

    def check(self, g):
        out = {}
        for s in self.spaces:
            rows, hist, read = READS[s]
            ents = getattr(g, rows)()
            want = self.ref[s].window(ents, getattr(g, hist)())
            got = getattr(g, read)()
            assert got.shape == want.shape, (s, got.shape, want.shape)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert got.tobytes() == want.tobytes(), (s, bad[:4].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
            self.check_state(g, s)
            out[s] = (ents, got)
        return out

    def check_state(self, g, s):
        ref = self.ref[s]
        got, want = g.slo_entries(s), ref.entries()
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (s, got[:2].tolist(), want[:2].tolist())
        st, ws = g.slo_stats(s), ref.stats()
        assert tuple(getattr(st, k) for k in STATS) == tuple(ws[k] for k in STATS), s


def _twin_reads(g):
    calls = ["window_nodes", "window_groups", "window_group_nodes", "window_group_perm", "window_hist", "window_node_hist",
             "window_node_quantiles", "window_group_node_hist", "window_group_node_quantiles"]
    return {c: getattr(g, c)().tobytes() for c in calls}


# ---- 1. the churn: exact after every window, a twin without the stage unchanged ------------------------------------------------------
@pytest.mark.parametrize("S,L", [(1, 3), (3, 3), (2, 5)])
def test_churn_is_exact_and_a_twin_without_the_stage_is_unchanged(churn, S, L):
    """L + 3 windows: services that come and go (a group of edges is absent for one window, another for five), OBIP rows whose list
    index changes (untracked), alive-only rows, drifting latency and errors.  Every other output is the twin's byte for byte, K20's
    tables among them."""
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    g, twin = (_engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True) for _ in range(2))
    for x in (g, twin):
        _stages(x, gmap)
    slo = Slo(g, mk, **{**PARAMS, "short_windows": S, "long_windows": L})
    burning = untracked = 0
    for w in wins[:L + 3]:
        _feed(g, _thin(w)); _feed(twin, _thin(w))
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        a, b = _twin_reads(g), _twin_reads(twin)
        for c in a:
            assert a[c] == b[c], c
        t = slo.check(g)
        for s in BOTH:
            ents, rows = t[s]
            burning += int(((rows[:, 16] & np.uint64(30)) != 0).sum())
            untracked += int((rows[:, 16] & np.uint64(1)).sum())
            assert (((rows[:, 16] & np.uint64(1)) != 0) == ((ents["ref"] >> 30) == 2)).all()   # exactly the OBIP rows
    assert burning > 0 and untracked > 0
    st = g.slo_stats("nodes")
    assert st.windows == L + 3 and 0 < st.keys_active < st.keys


def test_sixty_four_windows_long_span_with_seventy_tiny_windows(churn):
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    g = _engine(topo, labels, variant=2, max_edges=1 << 12, edge_histogram=True)
    _stages(g, _map("blocks", mk, topo.n_pods))
    slo = Slo(g, mk, **{**PARAMS, "short_windows": 5, "long_windows": 64, "min_requests": 100})
    for i in range(70):
        _feed(g, wins[i % 12][(i % 7)::96])
        g.flush_window()
        if i % 9 == 0 or i >= 62:
            slo.check(g)
        else:                                                         # (the reference follows every window; the rows are read at some)
            for s in BOTH:
                slo.ref[s].window(getattr(g, READS[s][0])(), getattr(g, READS[s][1])())
    rows = g.window_node_slo()
    assert (rows[(rows[:, 16] & np.uint64(1)) == 0][:, 17] == np.uint64(5 | 64 << 32)).all()   # both spans are full


# ---- 2. k1_variant 0 / 1 / 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_k1_variants(churn, variant):
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    g = _engine(topo, labels, variant=variant, max_edges=1 << 13, edge_histogram=True)
    _stages(g, _map("blocks", mk, topo.n_pods))
    slo = Slo(g, mk, **PARAMS)
    for w in wins[:4]:
        _feed(g, _thin(w))
        g.flush_window()
        t = slo.check(g)
    assert (t["group_nodes"][1][:, 3] > 0).any()


# ---- 3. constructed windows ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def small():
    topo, g, mk = _pods_engine(n_pods=40, edge_histogram=True)
    g.set_label_count(16)
    gmap = np.full(mk, NO, np.uint32); gmap[:8] = 0                   # workload 0 = pods 0 .. 7
    _stages(g, gmap)
    return topo, g, mk


SMALL = dict(latency_bin=3, latency_target_ppm=900_000, error_target_ppm=990_000, short_windows=2, long_windows=4, min_burn_q10=1024,
             min_requests=4)


def _row(g, space, ref):
    ents = getattr(g, READS[space][0])()
    return getattr(g, READS[space][2])()[int(np.flatnonzero(ents["ref"] == ref)[0])]


def test_a_service_goes_silent_and_returns_and_a_burst_leaves_the_short_span_first(small):
    """pod 21 receives 6 requests a window, all failing in window 0 (the burst), then goes silent for windows 3 .. 5 and returns: the
    burst is in the short span (S = 2) for windows 0 and 1, in the long one (L = 4) until window 3, and after the silence nothing
    of it is left"""
    topo, g, mk = small
    slo = Slo(g, mk, ml=16, **SMALL)
    src, dst = np.arange(10, 16), np.full(6, 21)
    seen = []
    for w in range(8):
        if 3 <= w <= 5:
            _send(topo, g, [30], [31])                                # (pod 21 has no row)
        else:
            _send(topo, g, src, dst, status=503 if w == 0 else 200)
        slo.check(g)
        if not 3 <= w <= 5:
            r = _row(g, "nodes", 21)
            seen.append((w, int(r[0]), int(r[1]), int(r[3]), int(r[4]), int(r[16]) & 2))
    assert seen[:3] == [(0, 6, 6, 6, 6, 2), (1, 12, 6, 12, 6, 2), (2, 12, 0, 18, 6, 0)]   # window 2: out of the short span, still in the long one
    assert seen[3:] == [(6, 6, 0, 6, 0, 0), (7, 12, 0, 12, 0, 0)]     # windows 3 .. 5 retired everything while the key had no row
    e = g.slo_entries("nodes")
    assert 21 in e[:, 0].tolist()


def test_keys_at_the_bounds_obip_rows_a_self_loop_alive_only_rows_and_an_empty_window(small):
    topo, g, mk = small
    g.upsert_pod(0x0A7F0001, mk - 1)                                  # the last KNOWN key
    slo = Slo(g, mk, ml=16, **SMALL)
    none = np.zeros(0, np.int64)
    _send(topo, g, none, none)                                        # an empty window first
    t = slo.check(g)
    assert all(len(t[s][1]) == 0 and len(g.slo_entries(s)) == 0 and g.slo_stats(s).windows == 1 for s in BOTH)
    pod = _events(topo, [9, 9, 9, 12, 12], topo.pod_ips[[9, 9, 9, 13, 14]])          # pod 9 calls itself: a self-loop
    last = _events(topo, [1, 1], topo.pod_ips[[20, 20]]); last["saddr"] = 0x0A7F0001   # the pod with node id mk - 1
    ext = _events(topo, [15, 16, 17, 17], EXT + np.arange(4, dtype=np.uint32), label=[1, 16, 0, 0])   # labels 0 and 15, two raw addresses
    alive = _events(topo, [18], topo.pod_ips[[19]], alive=[True])
    for w in range(3):
        g.ingest_bulk(np.concatenate([pod, last, ext, alive])); g.flush_window()
        t = slo.check(g)
        ents, rows = t["nodes"]
        refs = ents["ref"].tolist()
        for r in (mk - 1, LABEL | 0, LABEL | 15, 9, 18, 19):
            assert r in refs, r
        ob = ents["ref"] >> 30 == 2
        assert ob.sum() == 2 and (rows[ob, 16] == 1).all() and (rows[ob][:, :16] == 0).all() and (rows[ob, 17] == 0).all()
        self_loop = rows[refs.index(9)]
        assert int(self_loop[0]) == int(self_loop[8]) == 3 * min(w + 1, 2)          # both sides of pod 9 count its three calls
        idle = rows[refs.index(18)]
        assert int(idle[16]) == 0 and (idle[:16] == 0).all() and int(idle[17]) == (min(w + 2, 2) | min(w + 2, 4) << 32)   # tracked, no request
    keys = g.slo_entries("nodes")[:, 0].tolist()
    assert mk - 1 in keys and mk in keys and mk + 15 in keys and 18 not in keys
    wkeys = g.slo_entries("group_nodes")[:, 0].tolist()
    assert 2 * mk - 1 in wkeys and 2 * mk in wkeys and 2 * mk + 15 in wkeys


@pytest.mark.parametrize("lbin", [0, 14])
def test_latency_bin_zero_and_fourteen_on_both_sides_of_the_octave(small, lbin):
    """a request is slow from the lower edge of bin latency_bin + 1 on: 2^(17 + latency_bin) ns"""
    topo, g, mk = small
    slo = Slo(g, mk, ml=16, **{**SMALL, "latency_bin": lbin})
    edge = 1 << (17 + lbin)
    _send(topo, g, [10, 11, 12, 13], [20, 20, 21, 21], dur=[edge - 1, edge - 1, edge, edge + 1])
    slo.check(g)
    assert int(_row(g, "nodes", 20)[2]) == 0 and int(_row(g, "nodes", 21)[2]) == 2
    assert int(_row(g, "nodes", 12)[10]) == 1 and int(_row(g, "nodes", 10)[10]) == 0   # the callers' out sides


def test_a_rollout_keeps_the_workloads_sums_while_every_pod_key_is_new(small):
    topo, g, mk = small
    slo = Slo(g, mk, ml=16, **SMALL)
    old, new, dst = np.repeat(np.arange(0, 4), 3), np.repeat(np.arange(4, 8), 3), np.tile(np.arange(20, 23), 4)
    for w in range(2):
        _send(topo, g, old, dst, status=503)
        slo.check(g)
    _send(topo, g, new, dst)
    t = slo.check(g)
    wl = _row(g, "group_nodes", G(0))
    assert (int(wl[8]), int(wl[9]), int(wl[11]), int(wl[12])) == (24, 12, 36, 24)   # the out side: T_S, E_S, T_L, E_L across the rollout
    ents, rows = t["nodes"]
    fresh = rows[np.isin(ents["ref"], np.arange(4, 8))]
    assert (fresh[:, 8] == 3).all() and (fresh[:, 11] == 3).all() and (fresh[:, 9] == 0).all()


def test_objectives_before_and_between_windows_and_their_reset(small):
    topo, g, mk = small
    slo = Slo(g, mk, ml=16, **SMALL)
    strict = engine.slo_objective(1, 999_000, 999_900)               # a lower bin and two tighter budgets
    slo.assign(g, "nodes", [21], [strict])
    slo.assign(g, "group_nodes", [G(0), 21], [strict, engine.slo_objective(14, 500_000, 900_000)])
    src, dst = np.array([0, 1, 10, 11]), np.array([21, 21, 21, 22])
    _send(topo, g, src, dst, status=[503, 200, 200, 200], dur=1 << 19)   # bin 3: slow under the strict objective only
    slo.check(g)
    r = _row(g, "nodes", 21)
    assert int(r[16]) >> 32 == strict and int(r[2]) == 3 and int(_row(g, "nodes", 22)[2]) == 0 and int(_row(g, "nodes", 22)[16]) >> 32 == 0
    assert int(_row(g, "group_nodes", G(0))[10]) == 2                 # workload 0's out side, judged by the strict bin
    slo.assign(g, "nodes", [21, 22], [0, strict])                     # between windows: 21 back to the defaults
    _send(topo, g, src, dst, status=[503, 200, 200, 200], dur=1 << 19)
    slo.check(g)
    r = _row(g, "nodes", 21)
    assert int(r[16]) >> 32 == 0 and int(r[2]) == 3                   # history stays: the first window's three slow requests
    assert int(_row(g, "nodes", 22)[2]) == 1
    for refs, obj in (([G(0)], [strict]), ([2 << 30], [strict]), ([mk], [strict]), ([LABEL | 16], [strict]), ([21], [15 << 28 | 1 << 12 | 1]),
                      ([21], [1 << 24 | 1 << 12 | 1]), ([21], [1 << 12]), ([21], [1001 << 12 | 1]), ([21], [3 << 22 | 1000 << 12 | 1])):
        assert _rc(g.slo_assign, "nodes", refs, obj) == engine.SG_EINVAL
    assert _rc(g.slo_assign, "group_nodes", [G(mk)], [strict]) == engine.SG_EINVAL
    assert _rc(g.slo_assign, 3, [21], [strict]) == engine.SG_EINVAL
    slo.check_state(g, "nodes")                                       # a refused call set nothing


# ---- 4. every close path ----------------------------------------------------------------------------------------------------------------
def test_every_close_path(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    g.set_trend(shift=3, warmup=1)                                    # (for the _top_by flush)
    slo = Slo(g, mk, **PARAMS)
    for i, w in enumerate(wins[:8]):
        _feed(g, _thin(w))
        if i == 0:
            g.flush_begin()
            for call in (g.window_node_slo, g.window_group_node_slo, g.set_slo, g.window_nodes_top_slo, g.window_group_nodes_top_slo):
                assert _rc(call, *((1,) if "top" in call.__name__ else ())) == engine.SG_ESTATE     # a flush is open
            assert _rc(g.slo_assign, "nodes", [1], [0]) == engine.SG_ESTATE
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
        slo.check(g)


# ---- 5. three windows in flight ------------------------------------------------------------------------------------------------------------
def test_window_run_three_in_flight_through_the_device_buffers(churn):
    import torch
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True, windows_in_flight=3)
    one = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    gmap = _map("blocks", mk, topo.n_pods)
    for x in (g, one):
        _stages(x, gmap)
    slo = Slo(one, mk, **PARAMS)
    g.set_slo(BOTH, **PARAMS)
    hip = _hip()
    thin = [np.ascontiguousarray(_thin(w)) for w in wins[:6]]
    dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in thin]
    torch.cuda.synchronize()
    pending, sizes = [], []
    for i, w in enumerate(thin):
        _feed(one, w)
        one.flush_window()
        t = slo.check(one)
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((t, [g.window_slo_buffer(s) for s in BOTH]))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for t, bufs in pending:
                for s, p in zip(BOTH, bufs):
                    want = t[s][1]
                    assert _d2h(hip, p, want.nbytes, np.uint8).tobytes() == want.tobytes(), s
                sizes.append(len(t["nodes"][0]))
            pending = []
    assert len(sizes) == 6 and len(set(sizes)) > 1
    for s in BOTH:                                                    # the state updates ran in window order
        assert g.slo_entries(s).tobytes() == slo.ref[s].entries().tobytes()
        assert g.slo_stats(s).windows == 6


# ---- 6. the selections ----------------------------------------------------------------------------------------------------------------------
def test_the_selections_against_the_reference_ranking_with_ties(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    _stages(g, _map("blocks", mk, topo.n_pods))
    slo = Slo(g, mk, **PARAMS)
    for w in wins[:3]:
        _feed(g, _thin(w))
        g.flush_window()
        t = slo.check(g)
    for s, top in (("nodes", g.window_nodes_top_slo), ("group_nodes", g.window_group_nodes_top_slo)):
        ents, rows = t[s]
        for by in engine.SLOSEL_BY:
            for side in engine.SLOSEL_SIDE:
                vals = np.array(slo_values(rows, by, side, PARAMS["min_requests"]))
                assert (vals > 0).any() and len(set(vals.tolist())) < len(vals)       # something burns, and there are ties
                mid = int(np.sort(vals[vals > 0])[(vals > 0).sum() // 2])
                for k in (0, 1, 7, len(ents) + 5):
                    for thr in (0, 1, mid, mid + 1, 1 << 31):
                        want = ref_select_slo(rows, by, side, k, thr, PARAMS["min_requests"])
                        got, idx, n = top(k, thr, by=by, side=side)
                        assert n == len(ents) and idx.tolist() == want.tolist(), (s, by, side, k, thr)
                        assert got.tobytes() == ents[want].tobytes()
    for bad in (1, 6, 7, 8, 3 | 8):                                   # no side, both sides, an unknown bit
        assert g._l.sg_window_nodes_top_slo(g._h, bad, 1, 0, None, None, 0, None, None) == engine.SG_EINVAL
    assert g._l.sg_window_group_nodes_top_slo(g._h, 2, engine.SELECT_MAX_K + 1, 0, None, None, 0, None, None) == engine.SG_EINVAL


# ---- 7. lifecycle and return codes ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2, max_edges=1 << 13, edge_histogram=True)
    mk = topo.n_nodes + 8
    assert _rc(g.set_slo, "nodes", **PARAMS) == engine.SG_ESTATE      # K20 has no space on
    g.set_nodes(); g.set_quantiles("nodes")
    assert _rc(g.set_slo, "group_nodes", **PARAMS) == engine.SG_ESTATE and _rc(g.set_slo, BOTH, **PARAMS) == engine.SG_ESTATE
    for bits in (2, 3, 8):
        assert _rc(g.set_slo, bits, **PARAMS) == engine.SG_EINVAL     # unknown space bits (SG_Q_GROUPS has no SLO state)
    for bad in (dict(latency_bin=15), dict(latency_target_ppm=0), dict(latency_target_ppm=1_000_000), dict(error_target_ppm=0),
                dict(error_target_ppm=1_000_000), dict(short_windows=0), dict(short_windows=6), dict(long_windows=65, short_windows=65),
                dict(long_windows=65), dict(reserved=1)):
        assert _rc(g.set_slo, "nodes", **{**PARAMS, **bad}) == engine.SG_EINVAL, bad
    for call in (g.window_node_slo, g.window_group_node_slo):
        assert _rc(call) == engine.SG_ESTATE                          # off
    for s in BOTH:
        assert _rc(g.slo_entries, s) == engine.SG_ESTATE and _rc(g.slo_stats, s) == engine.SG_ESTATE and _rc(g.window_slo_buffer, s) == engine.SG_ESTATE
        assert _rc(g.slo_assign, s, [1], [0]) == engine.SG_ESTATE
    for bad in (0, 2, 5, 8):
        assert _rc(g.window_slo_buffer, bad) == engine.SG_EINVAL and _rc(g.slo_entries, bad) == engine.SG_EINVAL
        assert _rc(g.slo_stats, bad) == engine.SG_EINVAL and _rc(g.slo_assign, bad, [1], [0]) == engine.SG_EINVAL
    assert _rc(g.window_nodes_top_slo, 1) == engine.SG_ESTATE and _rc(g.window_group_nodes_top_slo, 1) == engine.SG_ESTATE
    _feed(g, _thin(wins[0])); g.flush_window()
    slo = Slo(g, mk, spaces=("nodes",), **PARAMS)
    assert _rc(g.window_node_slo) == engine.SG_ESTATE                 # the last read window was closed while the stage was off
    assert _rc(g.window_nodes_top_slo, 1) == engine.SG_ESTATE and _rc(g.window_slo_buffer, "nodes") == engine.SG_ESTATE
    assert len(g.slo_entries("nodes")) == 0 and g.slo_stats("nodes").windows == 0
    _feed(g, _thin(wins[1])); g.flush_window()
    slo.check(g)
    assert _rc(g.window_node_slo, np.array([len(g.window_nodes())], np.uint32)) == engine.SG_EINVAL
    idx = np.array([3, 0, 3], np.uint32)
    assert g.window_node_slo(idx).tobytes() == g.window_node_slo()[idx].tobytes()
    assert _rc(g.window_group_node_slo) == engine.SG_ESTATE           # that space is not on
    g.set_slo("nodes", **PARAMS)                                      # every call starts empty state
    assert len(g.slo_entries("nodes")) == 0
    g.set_slo(None)                                                   # off
    assert _rc(g.slo_entries, "nodes") == engine.SG_ESTATE
    g.set_slo("nodes", **PARAMS); g.set_slo("nodes", None)            # params None: off
    assert _rc(g.slo_stats, "nodes") == engine.SG_ESTATE
    g.set_slo("nodes", **PARAMS)
    g.set_quantiles("nodes", (990, 500))                              # ANY sg_set_quantiles frees the stage in front of K20's tables
    assert _rc(g.slo_entries, "nodes") == engine.SG_ESTATE and _rc(g.window_node_slo) == engine.SG_ESTATE
    g.set_groups(); g.group_assign(np.arange(mk), _map("blocks", mk, topo.n_pods)); g.set_group_nodes()
    g.set_quantiles(BOTH)
    slo = Slo(g, mk, **PARAMS)
    _feed(g, _thin(wins[2])); g.flush_window()
    slo.check(g)
    g.set_group_nodes(False)                                          # a K20 space freed underneath: its SLO state goes, the other stays
    assert _rc(g.slo_entries, "group_nodes") == engine.SG_ESTATE and len(g.slo_entries("nodes"))
    g.set_nodes(False)
    assert _rc(g.slo_entries, "nodes") == engine.SG_ESTATE
