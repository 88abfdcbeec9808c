"""K12, the incidents (sg_set_incidents / sg_window_incidents / sg_window_node_incident / sg_window_incidents_buffer): the incident
rows and the incident per node row of every window against the pure-Python reference tests/incident_ref.py run on the same window's
rows, node rows, trend rows and rank rows — byte for byte, every field is an integer or a max of float bits — on every close path,
an engine with it against a twin without it, and constructed windows whose components are known."""
import ctypes as C

import numpy as np
import pytest

from alaz_amd import engine
from tests.gpu_scaffold import _check_incidents as _check, _d2h, _engine, _feed, _hip, _incident_close as _close, _incident_pods_engine as _pods_engine, _path, _rc
from tests.incident_ref import QUANTILES, incident_ref, quantile_threshold, row_values
from tests.nodes_ref import nodes_ref
from tests.traces import churn, warm_stream  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

INF = float("inf")
NO = engine.NO_INCIDENT
TREND = dict(shift=3, warmup=2, ttl=4)


@pytest.mark.parametrize("by,ranked", [("score", False), ("score", True), ("lat_dev", False), ("err_dev", True)])
def test_every_window_of_the_churn_is_exact(churn, by, ranked):
    """one engine per threshold — -inf, +inf and QUANTILES of the window's own values, taken from a twin that closes the window
    first (every engine sees every window once: the baselines agree)"""
    topo, labels, wins = churn
    specs = [-INF, INF] + list(QUANTILES)
    twin = _engine(topo, labels)
    gs = [_engine(topo, labels) for _ in specs]
    for x in [twin] + gs:
        x.set_nodes()
        if by != "score":
            x.set_trend(**TREND)
        if ranked:
            x.set_rank(iters=3)
    counts, sizes = set(), set()
    for w in wins:
        _feed(twin, w)
        ref_rows = twin.flush_window().copy()
        val = row_values(ref_rows, by, twin.window_trend() if by != "score" else None)
        for g, q in zip(gs, specs):
            thr = q if abs(q) == INF else quantile_threshold(val, q)
            g.set_incidents(by=by, min_value=thr)
            _feed(g, w)
            rows = g.flush_window().copy()
            assert rows.tobytes() == ref_rows.tobytes()
            got = _check(g, rows, by, thr)
            counts.add(len(got))
            sizes.add(int(got["nodes"].max()) if len(got) else 0)
            if q == INF:
                assert len(got) == 0
            if q == -INF:
                assert int(got["edges"].sum()) == int((~np.isnan(val)).sum())
    assert 0 in counts and 1 in counts and max(counts) > 3 and max(sizes) >= 3, (counts, sizes)


def test_a_twin_without_it_is_unchanged(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    for x in (g, twin):
        x.set_nodes(); x.set_trend(**TREND); x.set_vanished(silent_windows=1, min_seen=1)
        x.set_node_trend(shift=3, warmup=2, ttl=3, max_entries=700); x.set_rank(iters=4)
    thr = 0.0
    for i, w in enumerate(wins):
        by = ("score", "lat_dev", "err_dev")[i % 3]
        g.set_incidents(by=by, min_value=thr)
        _feed(g, w); _feed(twin, w)
        rows = g.flush_window().copy()
        assert rows.tobytes() == twin.flush_window().tobytes()
        nodes = g.window_nodes()
        assert nodes.tobytes() == twin.window_nodes().tobytes() == nodes_ref(rows).tobytes()
        assert g.window_trend().tobytes() == twin.window_trend().tobytes()
        assert g.window_node_trend().tobytes() == twin.window_node_trend().tobytes()
        assert g.window_vanished().tobytes() == twin.window_vanished().tobytes()
        assert g.window_rank().tobytes() == twin.window_rank().tobytes()
        _check(g, rows, by, thr, nodes)
        nxt = ("score", "lat_dev", "err_dev")[(i + 1) % 3]
        thr = quantile_threshold(row_values(rows, nxt, g.window_trend()), 0.9)
    assert g.node_trend_entries().tobytes() == twin.node_trend_entries().tobytes()
    assert g.trend_entries().tobytes() == twin.trend_entries().tobytes()


def _run_windows(g, wins, ranked=False):
    """close `wins` on g, the threshold of each window the 0.9 score quantile of the one before it (-inf for the first)"""
    g.set_nodes()
    if ranked:
        g.set_rank(iters=3)
    thr, seen = -INF, []
    for w in wins:
        g.set_incidents(min_value=thr)
        _feed(g, w)
        s0 = g.stats()
        rows = g.flush_window().copy()
        seen.append(_path(s0, g.stats()))
        _check(g, rows, "score", thr)
        thr = quantile_threshold(rows["score"], 0.9)
    return seen


def test_warm_delta_and_cold_windows(warm_stream):
    topo, labels, wins = warm_stream
    g = _engine(topo, labels, max_window_events=700_000)
    seen = _run_windows(g, wins, ranked=True)
    assert {"cold", "warm", "delta"} <= set(seen), seen


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_k1_variants(churn, variant):
    topo, labels, wins = churn
    _run_windows(_engine(topo, labels, variant=variant), wins[:5])


def test_histogram_engine(churn):
    topo, labels, wins = churn
    _run_windows(_engine(topo, labels, variant=2, edge_histogram=True), wins[:4], ranked=True)


def test_begin_end_view_top_and_index_gather(churn):
    topo, labels, wins = churn
    g, twin = _engine(topo, labels), _engine(topo, labels)
    g.set_nodes(); g.set_rank(iters=3)
    rng = np.random.default_rng(5)
    thr = -INF
    for i, w in enumerate(wins[:8]):
        g.set_incidents(min_value=thr)
        _feed(g, w); _feed(twin, w)
        full = twin.flush_window().copy()
        if i % 4 == 0:
            g.flush_begin()
            assert _rc(g.window_incidents) == engine.SG_ESTATE          # a flush is open
            assert _rc(g.window_node_incident) == engine.SG_ESTATE
            assert _rc(g.set_incidents) == engine.SG_ESTATE and _rc(g.set_incidents, None) == engine.SG_ESTATE
            rows = g.flush_end().copy()
        elif i % 4 == 1:
            rows = g.flush_window_view().copy()
        elif i % 4 == 2:
            g.flush_begin()
            rows = g.flush_end_view().copy()
        else:
            sel, idx, n_edges = g.flush_window_top(3)
            assert n_edges == len(full)
            rows = full
        assert rows.tobytes() == full.tobytes()
        got = _check(g, rows, "score", thr)
        inc = g.window_node_incident()
        idx = rng.integers(0, len(inc), 37).astype(np.uint32)
        assert g.window_node_incident(idx).tolist() == inc[idx].tolist()
        assert _rc(g.window_node_incident, np.array([len(inc)], np.uint32)) == engine.SG_EINVAL
        if len(got) > 1:                                              # cap smaller than *n: the first rows, the true count
            buf = np.zeros(1, engine.INCIDENT_DTYPE); n = C.c_size_t(0)
            assert g._l.sg_window_incidents(g._h, buf.ctypes.data, 1, C.byref(n)) == 0
            assert n.value == len(got) and buf.tobytes() == got[:1].tobytes()
            few = np.full(2, 7, np.uint32)
            assert g._l.sg_window_node_incident(g._h, None, 0, few.ctypes.data, 2, C.byref(n)) == 0
            assert n.value == len(inc) and few.tolist() == inc[:2].tolist()
        thr = quantile_threshold(rows["score"], (0.5, 0.9, 0.99)[i % 3])


def test_lifecycle_and_error_codes(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    assert _rc(g.set_incidents) == engine.SG_ESTATE                    # the rollup is off
    assert _rc(g.window_incidents) == engine.SG_ESTATE and _rc(g.window_incidents_buffer) == engine.SG_ESTATE
    assert _rc(g.window_node_incident) == engine.SG_ESTATE
    g.set_nodes()
    assert _rc(g.window_incidents) == engine.SG_ESTATE                 # the incidents are off
    for bad in (dict(by="new"), dict(by=4), dict(struct_size=12), dict(struct_size=20), dict(reserved=1)):
        assert _rc(g.set_incidents, **bad) == engine.SG_EINVAL
    assert _rc(g.set_incidents, by="lat_dev") == engine.SG_ESTATE      # a trend key, the trend off
    assert _rc(g.set_incidents, by="err_dev") == engine.SG_ESTATE
    _feed(g, wins[0]); g.flush_window()
    g.set_incidents(min_value=-INF)
    assert _rc(g.window_incidents) == engine.SG_ESTATE                 # the read window was closed before it was on
    assert _rc(g.window_node_incident) == engine.SG_ESTATE
    _feed(g, wins[1])
    _check(g, g.flush_window().copy(), "score", -INF)
    g.set_trend(**TREND)
    g.set_incidents(by="lat_dev", min_value=0.0)
    assert _rc(g.window_incidents) == engine.SG_ESTATE                 # new parameters: the windows from here on
    _feed(g, wins[2])
    _check(g, g.flush_window().copy(), "lat_dev", 0.0)
    g.set_trend(**TREND)                                               # a new baseline: the incidents stay on
    _feed(g, wins[3])
    _check(g, g.flush_window().copy(), "lat_dev", 0.0)
    g.set_trend(None)                                                  # the trend off takes incidents by a trend key with it
    assert _rc(g.window_incidents) == engine.SG_ESTATE and _rc(g.window_incidents_buffer) == engine.SG_ESTATE
    g.set_incidents(min_value=0.0)
    g.set_trend(**TREND); g.set_trend(None)                            # ... and leaves incidents by score alone
    _feed(g, wins[4])
    _check(g, g.flush_window().copy(), "score", 0.0)
    g.set_incidents(None)
    assert _rc(g.window_incidents) == engine.SG_ESTATE
    g.set_incidents()
    g.set_nodes(False)                                                 # the rollup off takes the incidents with it
    assert _rc(g.window_incidents) == engine.SG_ESTATE and _rc(g.set_incidents) == engine.SG_ESTATE
    g.set_nodes(True)
    _feed(g, wins[5]); g.flush_window()
    assert _rc(g.window_incidents) == engine.SG_ESTATE


def test_sharded_engine_is_refused():
    g = engine.ServiceGraph(max_known_nodes=1024, max_edges=4096, layers=1, max_labels=16, max_outbound_ips=64, rank=0, world=2)
    assert _rc(g.set_nodes, True) == engine.SG_EINVAL
    assert _rc(g.set_incidents) == engine.SG_ESTATE


@pytest.mark.parametrize("in_flight", [1, 3, 8])
def test_window_run_in_flight(churn, in_flight):
    """sg_window_run with windows in flight: each slot's incidents against its own window (the scratch is shared and chained); read
    only after all of a round of slots were enqueued, so that the groupings of several windows are queued behind each other"""
    import torch
    topo, labels, wins = churn
    g, one = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    one.set_nodes(); one.set_rank(iters=3)
    _feed(one, wins[0])
    thr = quantile_threshold(one.flush_window()["score"], 0.9)
    g.set_nodes(); g.set_rank(iters=3); g.set_incidents(min_value=thr)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:9]]
    torch.cuda.synchronize()
    pending, counts = [], set()
    for i, w in enumerate(wins[:9]):
        _feed(one, w)
        rows = one.flush_window().copy()
        nodes, rank = one.window_nodes(), one.window_rank()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        pending.append((rows, nodes, rank, g.window_incidents_buffer()))
        if len(pending) == in_flight or i == 8:
            torch.cuda.synchronize()
            for rows, nodes, rank, (ip, cp, np_) in pending:
                cnt = int(_d2h(hip, cp, 1, np.uint64)[0])
                want, winc = incident_ref(rows, nodes, "score", thr, rank=rank)
                assert cnt == len(want)
                assert _d2h(hip, ip, cnt, engine.INCIDENT_DTYPE).tobytes() == want.tobytes()
                assert _d2h(hip, np_, len(nodes), np.uint32).tobytes() == winc.tobytes()
                counts.add(cnt)
            pending = []
    assert max(counts) > 3


def test_window_run_and_read(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels, variant=2)
    g.set_nodes(); g.set_incidents(min_value=-INF)
    for w in wins[:3]:
        _feed(g, w)
        g.window_run()
        _check(g, g.window_read().copy(), "score", -INF)


# ---- constructed windows with known answers: pod-to-pod events only and min_value = -inf, so every row is red ---------------------


@pytest.mark.parametrize("max_known", [None, 40_000])
def test_64_disjoint_chains(max_known):
    """chains of 1 .. 64 hops over pods whose ids are a seeded permutation: the incidents are exactly the chains"""
    n = sum(h + 1 for h in range(1, 65))
    topo, g = _pods_engine(n, max_known)
    perm = np.random.default_rng(64).permutation(n)
    src, dst, chains, at = [], [], [], 0
    for h in range(1, 65):
        ids = perm[at:at + h + 1]; at += h + 1
        src += ids[:-1].tolist(); dst += ids[1:].tolist()
        chains.append(sorted(ids.tolist()))
    rows, nodes, got, inc = _close(topo, g, src, dst)
    assert nodes["ref"].tolist() == list(range(n)) and len(got) == 64
    chains.sort()                                                     # by their smallest pod: the incidents' numbering
    for i, ids in enumerate(chains):
        assert got["first_node"][i] == ids[0] and got["nodes"][i] == len(ids) and got["edges"][i] == len(ids) - 1
        assert np.flatnonzero(inc == i).tolist() == ids
        assert got["count"][i] == len(ids) - 1
    assert int(got["err"].sum()) == int(rows["err_count"].sum()) > 0


@pytest.mark.parametrize("max_known", [None, 40_000])
@pytest.mark.parametrize("order", ["permuted", "descending"])
def test_one_chain_of_4097_pods(order, max_known):
    """deep trees, and roots that move across many workgroups"""
    n = 4097
    topo, g = _pods_engine(n, max_known)
    ids = np.random.default_rng(4097).permutation(n) if order == "permuted" else np.arange(n)[::-1]
    rows, nodes, got, inc = _close(topo, g, ids[:-1], ids[1:])
    assert len(got) == 1 and (got["first_node"][0], got["nodes"][0], got["edges"][0], got["count"][0]) == (0, n, n - 1, n - 1)
    assert (inc == 0).all() and len(inc) == n


@pytest.mark.parametrize("max_known", [None, 40_000])
def test_one_pod_calling_5000_others(max_known):
    """every hook lands on one root"""
    n = 5001
    topo, g = _pods_engine(n, max_known)
    hub = 2500
    others = np.array([i for i in range(n) if i != hub])
    rows, nodes, got, inc = _close(topo, g, np.full(n - 1, hub), others)
    assert len(got) == 1 and (got["first_node"][0], got["nodes"][0], got["edges"][0]) == (0, n, n - 1)
    assert (inc == 0).all()
    assert got["top_node"][0] == int(np.flatnonzero(nodes["score"] == nodes["score"].max())[0])


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_node_row_counts_around_the_node_span(n):
    """n node rows in red pairs and one triple: plan_incidents gives k12_label / k12_number 256 node rows a workgroup (any node
    capacity up to 262 144), so the incidents' heads lie on either side of a workgroup's rows"""
    topo, g = _pods_engine(600)
    ids = 50 + np.arange(n)
    src = ids[:-1][::2] if n % 2 == 0 else np.concatenate([ids[:-1][::2], [ids[-2]]])
    rows, nodes, got, inc = _close(topo, g, src, src + 1)
    assert len(nodes) == n and len(got) == n // 2
    assert got["first_node"].tolist() == list(range(0, 2 * (n // 2), 2))


def test_more_incidents_through_one_workgroup_of_the_rows_pass_than_its_table_has_slots():
    """max_edges 4096 over 8200 pods: 4096 disjoint red pairs 2i -> 2i + 1 are 4096 incidents; each of the four workgroups of
    k12_rows takes 1024 rows — 1024 distinct incidents against 512 table slots (tests/test_incident_host.py holds the plan to
    that), and no wave names one incident.  Ranked: the culprit loop runs beside it"""
    # (k12_nodes' direct path is out of reach here: its grid is one round of 256 node rows a workgroup up to 262 144 node rows, 128
    #  pairs against 512 slots.  The node fold is one body for both spaces, and K18's instance takes eight rounds a workgroup in
    #  tests/test_gpu_group_incidents.py::test_more_incidents_through_one_workgroup_than_its_table_has_slots: its direct path runs there)
    topo, g = _pods_engine(8200, max_edges=4096)
    src = 2 * np.arange(4096)
    rows, nodes, got, inc = _close(topo, g, src, src + 1)
    assert len(got) == 4096 and (got["nodes"] == 2).all() and (got["edges"] == 1).all()
    assert got["worst_row"].tolist() == list(range(4096))
    assert inc.tolist() == np.repeat(np.arange(4096), 2).tolist()
    assert (got["culprit_node"] != NO).all()
