"""K15, the workload baselines (sg_set_group_trend / sg_window_group_trend / sg_group_trend_entries / sg_set_group_vanished /
sg_window_group_vanished / sg_window_groups_top / sg_window_groups_select and their *_buffer calls): the group trend rows, the whole
workload baseline, its statistics, the vanished workload dependencies and the selections of every window against the numpy
references of tests/group_trend_ref.py, run on the device's own window_groups() and outbound_ips() of that window — byte for byte,
as K8's and K10's — on every close path, across a rollout (where the pod-level baseline forgets and this one does not), across a
regrouping, at the boundaries of the merge, and an engine with it against a twin without it."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.gpu_scaffold import _d2h, _engine, _feed, _grouped, _hip, _map, _pairs, _path, _pods_engine, _rc
from tests.group_ref import group_ref
from tests.group_trend_ref import GroupTrendRef, GroupVanishRef, ref_select_groups
from tests.helpers import CLOCK, HostShim
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)
from tests.vanish_ref import NO_ROW

pytestmark = pytest.mark.gpu

ME = 1 << 15                                                          # max_edges of _engine
NO = engine.NO_GROUP
PARAMS = dict(shift=3, warmup=2, ttl=3)
STATS = ("windows", "entries", "inserted", "expired", "dropped")
INF = float("inf")


def _check(g, ref, van=None):
    """the last read window against ref (a GroupTrendRef; with van its GroupVanishRef) over the device's own group edges: the trend
    rows, the baseline, the statistics and the vanished list"""
    ge, ob = g.window_groups(), g.outbound_ips()
    if van is None:
        want = ref.window(ge, ob)
    else:
        want, lst, n = van.window(ge, ob)
        got, cnt = g.window_group_vanished(with_count=True)
        assert cnt == n and got.tobytes() == lst.tobytes()
    got = g.window_group_trend()
    assert len(got) == len(ge) and got.tobytes() == want.tobytes()
    assert g.group_trend_entries().tobytes() == ref.entries.tobytes()
    s = g.group_trend_stats()
    assert tuple(getattr(s, k) for k in STATS) == tuple(ref.stats[k] for k in STATS)
    return ge, want


# ---- 1. the churn ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def caps(churn, oracle_lib):
    """max_entries per map kind, chosen on the CPU: the reference without a capacity cut over the oracle's rows of the churn, under
    each map — four fifths of the entries its first window makes, so the first window already drops new entries"""
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    W = weights.make_weights(2)
    mk = topo.n_nodes + 8
    o.packed(wins[0], labels)
    o.window_close(W, 2)
    rows, ob = o.edge_rows(), o.outbound_ips()
    out = {}
    for kind in ("none", "blocks", "one"):
        ref = GroupTrendRef(ME, **PARAMS)
        ref.window(group_ref(rows, _map(kind, mk, topo.n_pods), mk, mk, 256)[0], ob)
        out[kind] = max(1, len(ref.entries) * 4 // 5)
    return out


@pytest.mark.parametrize("kind", ["none", "blocks", "one"])
def test_churn_is_exact_and_a_twin_without_it_is_unchanged(churn, caps, kind):
    topo, labels, wins = churn
    (g, gmap, mk), (twin, _, _) = _grouped(topo, labels, kind), _grouped(topo, labels, kind)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(shift=3, warmup=2, ttl=4); x.set_vanished(silent_windows=1, min_seen=1)
        x.set_node_trend(shift=3, warmup=2, ttl=3, max_entries=700)
    g.set_group_trend(max_entries=caps[kind], **PARAMS)
    ref = GroupTrendRef(ME, max_entries=caps[kind], **PARAMS)
    dev_seen = 0
    for w in wins:
        _feed(g, w); _feed(twin, w)
        assert g.flush_window().tobytes() == twin.flush_window().tobytes()
        ge, t = _check(g, ref)
        assert ge.tobytes() == twin.window_groups().tobytes()
        assert g.window_row_group().tobytes() == twin.window_row_group().tobytes()
        assert g.window_group_perm().tobytes() == twin.window_group_perm().tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_node_trend().tobytes() == twin.window_node_trend().tobytes()
        assert g.window_vanished().tobytes() == twin.window_vanished().tobytes()
        dev_seen += int((t["lat_dev"] != 0).sum() + (t["err_dev"] != 0).sum())
    assert g.trend_entries().tobytes() == twin.trend_entries().tobytes()
    assert ref.stats["dropped"] > 0 and dev_seen > 0
    if kind != "one":
        assert ref.stats["expired"] > 0


# ---- 2. every close path ---------------------------------------------------------------------------------------------------------
def test_warm_delta_and_cold_windows_across_workgroups(churn, warm_stream):
    """the default capacity (2 x max_edges entries): the merge of B + E elements is spread over 48 workgroups, spans cross them"""
    seen = {}
    for topo, labels, wins in (warm_stream, churn):
        g, gmap, mk = _grouped(topo, labels, "blocks", max_window_events=700_000)
        g.set_group_trend(shift=2, warmup=1, ttl=5)
        ref = GroupTrendRef(ME, shift=2, warmup=1, ttl=5)
        assert (ref.cap + ME + 2047) // 2048 == 48
        for w in wins:
            _feed(g, w)
            s0 = g.stats()
            g.flush_window()
            p = _path(s0, g.stats())
            seen[p] = seen.get(p, 0) + 1
            _check(g, ref)
    assert seen.get("cold", 0) > 0 and seen.get("warm", 0) > 0 and seen.get("delta", 0) > 0, seen


def test_every_close_path_updates_the_baseline_once(churn):
    topo, labels, wins = churn
    g, gmap, mk = _grouped(topo, labels, "blocks")
    g.set_group_trend(**PARAMS); g.set_group_vanished(silent_windows=1, min_seen=1)
    ref = GroupTrendRef(ME, **PARAMS)
    van = GroupVanishRef(ref, silent_windows=1, min_seen=1)
    for i, w in enumerate(wins[:7]):
        _feed(g, w)
        if i == 0:
            g.flush_begin()
            for call in (g.window_group_trend, g.window_group_vanished, g.set_group_trend, g.set_group_vanished):
                assert _rc(call) == engine.SG_ESTATE                   # a flush is open
            assert _rc(g.set_group_trend, None) == engine.SG_ESTATE and _rc(g.window_groups_top, 1) == engine.SG_ESTATE
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
        _check(g, ref, van)
    assert g.group_trend_stats().windows == 7


def test_window_run_in_flight_updates_in_window_order(churn):
    """sg_window_run with three windows in flight: each window's device buffers, read after the round was enqueued, equal the
    reference run in window order over a one-call engine's group edges"""
    import torch
    topo, labels, wins = churn
    (g, gmap, mk), (one, _, _) = _grouped(topo, labels, "blocks", windows_in_flight=3), _grouped(topo, labels, "blocks")
    g.set_group_trend(**PARAMS); g.set_group_vanished(silent_windows=1, min_seen=1, max_rows=50)
    ref = GroupTrendRef(ME, **PARAMS)
    van = GroupVanishRef(ref, silent_windows=1, min_seen=1, max_rows=50)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending, vanished = [], 0
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        one.flush_window()
        ge = one.window_groups()
        want, lst, n = van.window(ge, one.outbound_ips())
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((ge, want, lst, n, g.window_group_trend_buffer(), g.window_group_vanished_buffer(), g.window_groups_buffer()))
        if len(pending) == 3:
            torch.cuda.synchronize()
            for ge, want, lst, n, tp, (vp, vcp), (ep, cp, _, _) in pending:
                assert int(_d2h(hip, cp, 1, np.uint64)[0]) == len(ge)
                assert _d2h(hip, ep, len(ge), engine.GROUP_EDGE_DTYPE).tobytes() == ge.tobytes()
                assert _d2h(hip, tp, len(ge), engine.TREND_DTYPE).tobytes() == want.tobytes()
                assert int(_d2h(hip, vcp, 1, np.uint64)[0]) == n
                assert _d2h(hip, vp, len(lst), engine.VANISHED_DTYPE).tobytes() == lst.tobytes()
                vanished += n
            pending = []
    assert vanished > 50
    assert g.group_trend_entries().tobytes() == ref.entries.tobytes()
    s = g.group_trend_stats()
    assert tuple(getattr(s, k) for k in STATS) == tuple(ref.stats[k] for k in STATS) and s.windows == 9


# ---- constructed windows: pod-to-pod events ---------------------------------------------------------------------------------------
def _send(topo, g, src, dst, dur=1_000_000, alive=None, status=None):
    """one request (or, where alive, one alive record) per (src pod, dst pod) pair, then the window's rows"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = topo.pod_ips[dst]
    e["status"] = 200 if status is None else status
    e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = dur
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    if alive is not None:
        a = np.asarray(alive, bool)
        e["flags"][a] = replay.EV_ALIVE
        e["status"][a] = 0; e["protocol"][a] = 0; e["duration_ns"][a] = 0
    if len(e):
        g.ingest_bulk(e)
    return g.flush_window().copy()


# ---- 3. the rollout ---------------------------------------------------------------------------------------------------------------
def test_a_rollout_resets_the_pod_baseline_and_not_the_workload_baseline():
    """workload 0 = pods 0..7 calls workload 1 = pods 20..22: its events come from pods 0..3 for warmup + 2 windows, then from pods
    4..7 with the latency stepped up — the pod-level rows are new dependencies and the old pods' edges vanish; the workload's group
    edge keeps its history, shows the step and nothing vanishes"""
    topo, g, mk = _pods_engine()
    warmup = 2
    g.set_groups(); g.group_assign(np.arange(8), 0); g.group_assign(np.arange(20, 23), 1)
    g.set_trend(shift=1, warmup=warmup); g.set_vanished(silent_windows=1, min_seen=1)
    g.set_group_trend(shift=1, warmup=warmup); g.set_group_vanished(silent_windows=1, min_seen=1)
    ref = GroupTrendRef(1 << 14, shift=1, warmup=warmup)
    van = GroupVanishRef(ref, silent_windows=1, min_seen=1)
    old, new = np.repeat(np.arange(0, 4), 3), np.repeat(np.arange(4, 8), 3)
    dst = np.tile(np.arange(20, 23), 4)
    other_s, other_d = _pairs(40, 60, 3)                              # steady traffic among ungrouped pods 30..69
    for w in range(warmup + 2):
        rows = _send(topo, g, np.concatenate([old, other_s + 30]), np.concatenate([dst, other_d + 30]))
        ge, t = _check(g, ref, van)
        assert len(g.window_vanished()) == 0 and len(g.window_group_vanished()) == 0
    assert (g.window_trend()["windows_seen"] == warmup + 1).all()
    rows = _send(topo, g, np.concatenate([new, other_s + 30]), np.concatenate([dst, other_d + 30]),
                 dur=np.concatenate([np.full(12, 5_000_000), np.full(60, 1_000_000)]))
    ge, t = _check(g, ref, van)
    pod_t = g.window_trend()
    mine = (rows["from_ref"] >= 4) & (rows["from_ref"] < 8)           # (a KNOWN ref is its id)
    assert mine.sum() == 12 and (pod_t["windows_seen"][mine] == 0).all() and (pod_t["lat_dev"][mine] == 0).all()
    assert (pod_t["windows_seen"][~mine] == warmup + 2).all()
    k = np.flatnonzero((ge["from_ref"] == ((3 << 30) | 0)) & (ge["to_ref"] == ((3 << 30) | 1)))
    assert len(k) == 1 and ge["count"][k[0]] == 12 and ge["from_nodes"][k[0]] == 4
    assert t["windows_seen"][k[0]] == warmup + 2 and t["base_mean_us"][k[0]] == np.float32(1000.0)
    assert t["lat_dev"][k[0]] == np.float32(4_000_000 / 1000)         # x = 5 ms against a mean of 1 ms with no deviation: the floor
    pv = g.window_vanished()                                          # the old pods' 12 edges, and no workload dependency
    assert len(pv) == 12 and sorted(set(pv["from_key"].tolist())) == [0, 1, 2, 3] and (pv["row"] == NO_ROW).all()
    assert len(g.window_group_vanished()) == 0
    new_rows, _, _ = g.window_groups_top(0, by="new")
    assert len(new_rows) == 0                                         # ... and none is a new dependency either


# ---- 4. regrouping ---------------------------------------------------------------------------------------------------------------
def test_regrouping_through_group_assign_alone():
    """the map changes between windows, the baseline is not touched: entries under keys that no longer occur go silent, are listed
    once as vanished (silent_windows = 2) and expire (ttl = 4); where alive-only traffic remains under an unchanged key, `row` names
    the count == 0 group edge"""
    topo, g, mk = _pods_engine()
    n = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(n), np.arange(n) // 7)
    p = dict(shift=2, warmup=1, ttl=4)
    g.set_group_trend(**p); g.set_group_vanished(silent_windows=2, min_seen=2, max_rows=40)
    ref = GroupTrendRef(1 << 14, **p)
    van = GroupVanishRef(ref, silent_windows=2, min_seen=2, max_rows=40)
    src, dst = _pairs(n, 3000, 41)
    quiet = (src // 7 < 5) & (dst // 7 < 5)                           # pairs inside pods 0..34: they keep their groups, and go alive-only
    counts, rows_named, before = [], 0, None
    for w in range(9):
        if w == 3:
            ids = np.arange(77, n)
            g.group_assign(ids, 30 + ids // 5)                        # pods 77.. (workloads 11..21) move to workloads 45..59
            before = ref.stats["expired"]
        _send(topo, g, src, dst, dur=1_000_000 + 50_000 * w, alive=quiet if w >= 3 else None)
        ge, t = _check(g, ref, van)
        lst, cnt = g.window_group_vanished(with_count=True)
        counts.append(cnt)
        rows_named += int((lst["row"] != NO_ROW).sum())
        if len(lst):
            named = lst[lst["row"] != NO_ROW]
            assert (ge["count"][named["row"]] == 0).all() and (ge["alive"][named["row"]] > 0).all()
    assert counts[:4] == [0, 0, 0, 0] and counts[4] > 40 and counts[5:] == [0, 0, 0, 0]   # once, silent_windows after the change; cut at max_rows
    assert rows_named >= 10                                           # (workloads 0 and 1 to workloads 0..4: within the first max_rows keys)
    assert ref.stats["expired"] - before >= counts[4]                 # then they expire (those with alive-only traffic too)


# ---- 5. selection ------------------------------------------------------------------------------------------------------------------
def _select_all(g, ge, tr, torch, bys):
    hip = _hip()
    cap = len(ge) + 9
    d_out = torch.zeros(cap * engine.GROUP_EDGE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    for by in bys:
        v = ge["score_max"] if by == "score" else tr["lat_dev" if by == "new" else by]
        mid = float(np.sort(v[np.isfinite(v)])[len(v) // 2])
        for k in (0, 1, 7, len(ge) + 5, engine.SELECT_MAX_K):
            for thr in (-INF, mid, INF):
                want = ref_select_groups(ge, tr, by, k, thr)
                if by != "new":
                    assert (thr != INF or len(want) == 0) and (thr != -INF or k or len(want) == len(ge) - int(np.isnan(v).sum()))
                rows, idx, n_groups = g.window_groups_top(k, thr, by=by)
                assert n_groups == len(ge) and idx.tolist() == want.tolist(), (by, k, thr)
                assert rows.tobytes() == ge[want].tobytes()
                if by != "score" and len(idx):
                    assert g.window_group_trend(idx).tobytes() == tr[idx].tobytes()
                g.window_groups_select(k, thr, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0, by=by)
                torch.cuda.synchronize()
                assert int(d_n.cpu()[0]) == len(want), (by, k, thr)
                assert d_idx.cpu().numpy()[:len(want)].astype(np.uint32).tolist() == want.tolist()
                assert d_out.cpu().numpy()[: len(want) * 80].tobytes() == ge[want].tobytes()
    return d_out, d_idx, d_n, cap


def test_selection_host_and_device_forms():
    import torch
    topo, g, mk = _pods_engine()
    n = topo.n_pods
    gmap = np.full(mk, NO, np.uint32)
    gmap[:90] = np.arange(90) // 6                                    # workloads 0..14; pods 90..149 ungrouped
    g.set_groups(); g.group_assign(np.arange(mk), gmap)
    g.set_group_trend(shift=2, warmup=1)
    ref = GroupTrendRef(1 << 14, shift=2, warmup=1)
    src, dst = _pairs(90, 1500, 9)
    iso_s, iso_d = np.arange(100, 140, 2), np.arange(101, 141, 2)     # twenty identical isolated pairs: equal scores, ties
    rng = np.random.default_rng(5)
    for w in range(3):
        keep = rng.random(len(src)) < 0.8                             # some group edges are new in the later windows
        dur = np.concatenate([(1_000_000 * (1 + w * rng.random(int(keep.sum())))).astype(np.uint64), np.full(20, 2_000_000, np.uint64)])
        st = np.concatenate([np.where(rng.random(int(keep.sum())) < 0.1 * w, 503, 200), np.full(20, 200)])
        s_, d_ = np.concatenate([src[keep], iso_s]), np.concatenate([dst[keep], iso_d])
        if w == 2:                                                    # pods 90..99 speak for the first time: new group edges
            s_, d_ = np.concatenate([s_, np.arange(90, 100)]), np.concatenate([d_, np.arange(0, 10)])
            dur, st = np.concatenate([dur, np.full(10, 3_000_000, np.uint64)]), np.concatenate([st, np.full(10, 200)])
        _send(topo, g, s_, d_, dur=dur, status=st)
        ge, tr = _check(g, ref)
    iso = ge[(ge["from_ref"] >= 100) & (ge["from_ref"] < 140)]
    assert len(iso) == 20 and len(set(iso["score_max"].tobytes()[i * 4:i * 4 + 4] for i in range(20))) == 1   # the ties
    assert (tr["lat_dev"] != 0).any() and (tr["err_dev"] != 0).any() and ((tr["windows_seen"] == 0) & (ge["count"] > 0)).any()
    d_out, d_idx, d_n, cap = _select_all(g, ge, tr, torch, ("score", "lat_dev", "err_dev", "new"))
    # rows only, indices only, and a cap below the selection
    g.window_groups_select(5, -INF, d_out.data_ptr(), 0, cap, d_n.data_ptr(), 0)
    torch.cuda.synchronize()
    want = ref_select_groups(ge, None, "score", 5, -INF)
    assert d_out.cpu().numpy()[: 5 * 80].tobytes() == ge[want].tobytes()
    rows, idx, _ = g.window_groups_top(0, cap=4)
    assert len(rows) == len(idx) == 4 and idx.tolist() == [0, 1, 2, 3] and rows.tobytes() == ge[:4].tobytes()
    # the score needs the groups only
    g.set_group_trend(None)
    _send(topo, g, np.concatenate([src, iso_s]), np.concatenate([dst, iso_d]))
    ge = g.window_groups()
    _select_all(g, ge, None, torch, ("score",))
    for by in ("lat_dev", "err_dev", "new"):
        assert _rc(g.window_groups_top, 1, by=by) == engine.SG_ESTATE
        assert _rc(g.window_groups_select, 1, 0.0, 0, d_idx.data_ptr(), cap, d_n.data_ptr(), by=by) == engine.SG_ESTATE


def test_a_selection_longer_than_the_staging_is_gathered_in_pieces():
    """k = 0 over more group edges than the SG_SELECT_MAX_K rows the host form stages: nothing grouped, one group edge per row"""
    topo, g, mk = _pods_engine(max_known=None)
    g.set_groups()
    E = engine.SELECT_MAX_K - 3                                       # max_edges of this engine is 2^14 = SG_SELECT_MAX_K ...
    rows = _send(topo, g, *_pairs(topo.n_pods, E, 77))
    ge = g.window_groups()
    assert len(ge) == E
    got, idx, n = g.window_groups_top(0)
    assert n == E and idx.tolist() == list(range(E)) and got.tobytes() == ge.tobytes()
    big = engine.ServiceGraph(max_known_nodes=mk, max_edges=1 << 15, layers=2, max_labels=16, max_outbound_ips=64, max_window_events=1 << 16,
                              max_batch=1 << 14)                      # ... so a second engine whose windows can exceed the staging
    big.set_clock(*CLOCK); big.load_weights(weights.make_weights(2))
    HostShim().apply(big, topo.k8s_ops()); big.set_label_count(0)
    big.set_groups()
    E = engine.SELECT_MAX_K + 1001
    _send(topo, big, *_pairs(topo.n_pods, E, 78))
    ge = big.window_groups()
    got, idx, n = big.window_groups_top(0)
    assert n == E == len(ge) and idx.tolist() == list(range(E)) and got.tobytes() == ge.tobytes()
    want = ref_select_groups(ge, None, "score", 0, float(np.median(ge["score_max"])))
    got, idx, n = big.window_groups_top(0, float(np.median(ge["score_max"])))
    assert idx.tolist() == want.tolist() and got.tobytes() == ge[want].tobytes()


# ---- 6. boundaries ----------------------------------------------------------------------------------------------------------------
def test_empty_and_alive_only_windows_on_either_side_of_the_merge():
    topo, g, mk = _pods_engine()
    n = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(n), np.arange(n) // 7)
    p = dict(shift=1, warmup=1, ttl=3)
    g.set_group_trend(**p); g.set_group_vanished(silent_windows=1, min_seen=1)
    ref = GroupTrendRef(1 << 14, **p)
    van = GroupVanishRef(ref, silent_windows=1, min_seen=1)
    src, dst = _pairs(n, 500, 6)
    none = np.zeros(0, np.int64)
    _send(topo, g, none, none)                                        # B = 0, E = 0: the first window after set_group_trend
    ge, t = _check(g, ref, van)
    assert len(ge) == 0 and len(g.group_trend_entries()) == 0 and g.group_trend_stats().windows == 1
    _send(topo, g, src, dst, alive=np.ones(500, bool))                # alive-only rows: samples that create nothing (B = 0, E > 0)
    ge, t = _check(g, ref, van)
    assert len(ge) > 0 and (ge["count"] == 0).all() and len(ref.entries) == 0
    _send(topo, g, src, dst)                                          # B = 0, E > 0: every entry is new
    ge, t = _check(g, ref, van)
    assert len(ref.entries) == len(ge) > 0 and (t["windows_seen"] == 0).all()
    _send(topo, g, none, none)                                        # B > 0, E = 0: everything vanishes, nothing expires yet
    ge, t = _check(g, ref, van)
    assert len(ge) == 0 and len(g.window_group_vanished()) == len(ref.entries) > 0
    assert g.window_groups_top(0)[2] == 0 and len(g.window_groups_top(3, by="lat_dev")[0]) == 0
    _send(topo, g, src, dst, alive=np.ones(500, bool))                # alive-only rows against B > 0: reported, not refreshed
    ge, t = _check(g, ref, van)
    assert (t["windows_seen"] == 1).all() and (t["lat_dev"] == 0).all()
    _send(topo, g, none, none)                                        # w - last = 3 = ttl: the baseline empties
    _check(g, ref, van)
    assert len(ref.entries) == 0 and ref.stats["expired"] > 0


def test_index_reads():
    topo, g, mk = _pods_engine()
    n = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(n), np.arange(n) // 2)   # 75 workloads: up to 5 550 group edges
    g.set_group_trend(shift=1, warmup=1)
    ref = GroupTrendRef(1 << 14, shift=1, warmup=1)
    src, dst = _pairs(n, 6000, 12)
    for w in range(2):
        _send(topo, g, src, dst, dur=1_000_000 * (w + 1))
        ge, t = _check(g, ref)
    N = len(ge)
    assert N > 1025
    assert len(g.window_group_trend(np.zeros(0, np.uint32))) == 0
    rep = np.array([5, 5, 0, N - 1, 5], np.uint32)
    assert g.window_group_trend(rep).tobytes() == t[rep].tobytes()
    assert _rc(g.window_group_trend, np.array([0, N], np.uint32)) == engine.SG_EINVAL
    long = np.random.default_rng(1).integers(0, N, 1025).astype(np.uint32)   # one element longer than the staging's first size
    assert g.window_group_trend(long).tobytes() == t[long].tobytes()
    longer = np.random.default_rng(2).integers(0, N, 3000).astype(np.uint32)
    assert g.window_group_trend(longer).tobytes() == t[longer].tobytes()
    out = np.full(5, 0xFF, np.uint8).repeat(16).view(engine.TREND_DTYPE)       # cap below the count: the first cap rows only
    cnt = C.c_size_t(0)
    assert g._l.sg_window_group_trend(g._h, rep.ctypes.data, 5, out.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == 5 and out[:3].tobytes() == t[rep[:3]].tobytes() and out[3:].tobytes() == b"\xff" * 32
    out = np.full(4, 0xFF, np.uint8).repeat(16).view(engine.TREND_DTYPE)
    assert g._l.sg_window_group_trend(g._h, None, 0, out.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == N and out[:3].tobytes() == t[:3].tobytes() and out[3:].tobytes() == b"\xff" * 16


def test_an_engine_with_64_bit_group_keys():
    topo, g, mk = _pods_engine(40_000)                                # GK = 40 000 + 40 080: 17 + 17 key bits
    n = topo.n_pods
    g.set_groups(); g.group_assign(np.arange(n), np.arange(n) // 7 * 1000)
    g.set_group_trend(shift=2, warmup=1); g.set_group_vanished(min_seen=1)
    ref = GroupTrendRef(1 << 14, shift=2, warmup=1)
    van = GroupVanishRef(ref, min_seen=1)
    for w in range(3):
        src, dst = _pairs(n, 4097, 20 + w)
        keep = src < (70 if w == 2 else n)                            # the last window: the workloads of pods 70.. call nobody
        _send(topo, g, src[keep], dst[keep], dur=1_000_000 * (w + 1))
        ge, t = _check(g, ref, van)
    assert (t["windows_seen"] > 0).any() and (t["lat_dev"] != 0).any() and len(g.window_group_vanished()) > 0
    assert int(ge["to_ref"].max() & 0x3FFFFFFF) == (n - 1) // 7 * 1000


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    reads = (g.window_group_trend, g.window_group_trend_buffer, g.group_trend_entries, g.group_trend_stats)
    vreads = (g.window_group_vanished, g.window_group_vanished_buffer)
    assert _rc(g.set_group_trend) == engine.SG_ESTATE and _rc(g.set_group_trend, None) == engine.SG_ESTATE      # the groups are off
    assert _rc(g.set_group_vanished) == engine.SG_ESTATE and _rc(g.window_groups_top, 1) == engine.SG_ESTATE
    for call in reads + vreads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_groups(); g.group_assign(np.arange(topo.n_pods), np.arange(topo.n_pods) // 7)
    assert _rc(g.set_group_vanished) == engine.SG_ESTATE               # the group trend is off
    for bad in (dict(shift=11), dict(max_entries=(1 << 31) + 1), dict(struct_size=36), dict(reserved=1)):
        assert _rc(g.set_group_trend, **bad) == engine.SG_EINVAL
    assert _rc(g.window_groups_top, 1) == engine.SG_ESTATE             # no window closed with the groups on yet
    g.set_group_trend(**PARAMS)
    for bad in (dict(silent_windows=3), dict(max_rows=2 * ME + 1), dict(struct_size=12)):
        assert _rc(g.set_group_vanished, **bad) == engine.SG_EINVAL
    assert _rc(g.window_group_trend) == engine.SG_ESTATE and _rc(g.window_group_trend_buffer) == engine.SG_ESTATE   # no window closed with it on
    assert len(g.group_trend_entries()) == 0 and g.group_trend_stats().windows == 0
    _feed(g, wins[0]); g.flush_window()
    assert len(g.window_group_trend()) == len(g.window_groups()) > 0 and len(g.group_trend_entries()) > 0
    for call in vreads:
        assert _rc(call) == engine.SG_ESTATE                           # the list is off
    g.set_group_vanished()
    for call in vreads:
        assert _rc(call) == engine.SG_ESTATE                           # the read window was closed before it was on
    assert g._l.sg_window_groups_top(g._h, 4, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL      # by > SG_SEL_NEW
    assert g._l.sg_window_groups_top(g._h, 0, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    d_n = C.c_uint64(0)
    assert g._l.sg_window_groups_select(g._h, 4, 1, 0.0, None, None, 0, C.addressof(d_n), None) == engine.SG_EINVAL
    assert g._l.sg_window_groups_select(g._h, 0, engine.SELECT_MAX_K + 1, 0.0, None, None, 0, C.addressof(d_n), None) == engine.SG_EINVAL
    assert g._l.sg_window_groups_select(g._h, 0, 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL   # no count word
    g.set_trend(); g.set_vanished(); g.set_trend(None)                # the edge trend and its list do not touch it
    g.group_assign([0, 1], [5, NO])                                   # nor does the map
    _feed(g, wins[1]); g.flush_window()
    assert g.group_trend_stats().windows == 2 and g.window_group_vanished(with_count=True)[1] >= 0   # (readable: closed with the list on)
    g.set_group_trend(**PARAMS)                                       # re-enabling starts empty, and switches the list off
    assert len(g.group_trend_entries()) == 0 and g.group_trend_stats().windows == 0
    assert _rc(g.window_group_trend) == engine.SG_ESTATE and _rc(g.window_group_vanished) == engine.SG_ESTATE
    assert len(g.window_groups_top(2)[0]) == 2                        # the score: the groups of the read window are still there
    assert _rc(g.window_groups_top, 2, by="lat_dev") == engine.SG_ESTATE   # ... its trend rows are not
    _feed(g, wins[2]); g.flush_window()
    ref = GroupTrendRef(ME, **PARAMS)
    _check(g, ref)
    assert _rc(g.window_group_vanished) == engine.SG_ESTATE
    g.set_group_trend(None)
    for call in reads:
        assert _rc(call) == engine.SG_ESTATE
    g.set_group_trend(**PARAMS); g.set_group_vanished()
    g.set_groups()                                                    # any sg_set_groups call takes the stage and its list with it
    for call in reads + vreads:
        assert _rc(call) == engine.SG_ESTATE
    assert _rc(g.set_group_vanished) == engine.SG_ESTATE
    _feed(g, wins[3]); g.flush_window()
    assert _rc(g.window_group_trend) == engine.SG_ESTATE and len(g.window_groups()) > 0
    g.set_group_trend(**PARAMS)
    g.set_groups(None)
    assert _rc(g.group_trend_stats) == engine.SG_ESTATE and _rc(g.set_group_trend) == engine.SG_ESTATE
