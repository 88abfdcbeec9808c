"""Event traces, random windows and configuration lines that several test modules share — numpy and alaz_amd.replay only, no engine and
no library, so the CPU tests can import them.  The fixtures are found by pytest in the namespace of the module that imports them
(by the name they are imported under): from tests.traces import churn  # noqa: F401."""
import numpy as np
import pytest

from alaz_amd import engine, replay
from alaz_amd.replay import EDGE_OUT_DTYPE

# configuration lines of the plan driver's engine-level stages (tests/plan_driver.py)
C2 = "max_known_nodes=1500 max_edges=66596 layers=1 max_labels=64 max_window_events=1000000 k1_variant=3"
C3 = "max_known_nodes=15000 max_edges=1254096 layers=2 max_labels=64 max_window_events=10000000"                  # the flagship shape
C5_SHARD = "max_known_nodes=150000 max_edges=785346 layers=2 max_labels=64 max_window_events=625000 flags=2"


def _drift(ev, i, rng):
    """window i's events with latency drifting up and a growing share of errors"""
    e = ev.copy()
    e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.15 * i)).astype(np.uint64)
    bad = rng.random(len(e)) < 0.02 * (i % 5)
    e["status"][bad & (e["protocol"] == 1)] = 503
    return e


@pytest.fixture(scope="module")
def churn():
    """12 windows over one topology: whole groups of edges (and so nodes) missing from some windows, raw outbound IPs that come and
    go (the outbound-IP list changes), Host labels, reversed events, alive-only records, latency and error drift"""
    topo = replay.make_topology(300, 6000, seed=81)
    ev, labels = replay.make_events(topo, 360_000, seed=82, mixed=True, with_raw_outbound=True, with_reverse=True)
    rng = np.random.default_rng(83)
    al = np.zeros(3000, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
    pick = rng.random(len(al))
    al["daddr"] = np.where(pick < 0.5, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))],
                           np.where(pick < 0.8, topo.pod_ips[rng.integers(0, topo.n_pods, len(al))], 0x5DB8D800 + rng.integers(0, 40, len(al)))).astype(np.uint32)
    group = ((ev["saddr"].astype(np.uint64) * 2654435761 + ev["daddr"].astype(np.uint64) * 40503) >> 7) % 6
    wins = []
    for i in range(12):
        part = ev[i * 30_000:(i + 1) * 30_000]
        gp = group[i * 30_000:(i + 1) * 30_000]
        keep = (gp != (i % 6)) & ((gp != 5) | (i < 4) | (i > 8))        # group i % 6 absent for one window; group 5 for five
        a = al[rng.random(len(al)) < 0.3]
        wins.append(np.concatenate([_drift(part[keep], i, rng), a]))
    return topo, labels, wins


# (imported as churn by the tests of the edge baselines, K8: tests/test_gpu_trend.py and the two that follow it)
@pytest.fixture(scope="module")
def trend_churn():
    """12 windows over one topology: whole groups of edges missing from some windows (they expire and come back), raw outbound IPs,
    Host labels, reversed events and open-connection (alive-only) records"""
    topo = replay.make_topology(300, 6000, seed=81)
    ev, labels = replay.make_events(topo, 360_000, seed=82, mixed=True, with_raw_outbound=True, with_reverse=True)
    rng = np.random.default_rng(83)
    al = np.zeros(3000, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
    pick = rng.random(len(al))
    al["daddr"] = np.where(pick < 0.5, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))],
                           np.where(pick < 0.8, topo.pod_ips[rng.integers(0, topo.n_pods, len(al))], 0x5DB8D800 + rng.integers(0, 40, len(al)))).astype(np.uint32)
    group = ((ev["saddr"].astype(np.uint64) * 2654435761 + ev["daddr"].astype(np.uint64) * 40503) >> 7) % 6
    wins = []
    for i in range(12):
        part = ev[i * 30_000:(i + 1) * 30_000]
        gp = group[i * 30_000:(i + 1) * 30_000]
        keep = (gp != (i % 6)) & ((gp != 5) | (i < 4) | (i > 8))        # group i % 6 absent for one window; group 5 for five
        a = al[rng.random(len(al)) < 0.3]
        wins.append(np.concatenate([part[keep], a]))
    return topo, labels, wins


@pytest.fixture(scope="module")
def warm_stream():
    """windows without raw outbound IPs: cold, warm (a subset), delta (another draw), warm, delta — with drift"""
    topo = replay.make_topology(400, 30_000, seed=91)
    (e0, labels), (e1, _), (e2, _) = (replay.make_events(topo, 150_000, seed=92 + k, fixed_labels=True) for k in range(3))
    rng = np.random.default_rng(97)
    wins = [_drift(w, i, rng) for i, w in enumerate([e0, e0[::3], e1, e0, e2, e1[::2], e0, e2[::2]])]
    return topo, labels, wins


def _random_rows(rng, mk, ml, n_rows):
    """canonical rows over Known, Label and outbound-IP refs with self-loops, NaN, -0.0, equal and negative scores, alive-only rows
    and sums that wrap"""
    def refs(n):
        t = rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint32), n)
        v = np.where(t == 0, rng.integers(0, mk, n), np.where(t == 1, rng.integers(0, ml, n), rng.integers(0, 40, n))).astype(np.uint32)
        return (t << np.uint32(30)) | v
    f = refs(n_rows) & np.uint32(0x3FFFFFFF)                          # a source is a pod
    t = np.where(rng.random(n_rows) < 0.05, f, refs(n_rows))
    pairs = np.unique(np.stack([f, t], 1), axis=0)
    r = np.zeros(len(pairs), dtype=EDGE_OUT_DTYPE)
    r["from_ref"], r["to_ref"] = pairs[:, 0], pairs[:, 1]
    s = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 1.0, -1.0, np.nan], dtype=np.float32), len(r))
    r["score"] = np.where(rng.random(len(r)) < 0.5, rng.random(len(r)).astype(np.float32), s).astype(np.float32)
    r["count"] = rng.integers(0, 1 << 32, len(r)); r["err_count"] = rng.integers(0, 1 << 20, len(r))
    r["sum_ns"] = rng.integers(0, 1 << 63, len(r), dtype=np.uint64) * np.uint64(2)
    r["sumsq_us"] = rng.integers(0, 1 << 63, len(r), dtype=np.uint64) * np.uint64(2)
    r["max_ns"] = rng.integers(0, 1 << 40, len(r)); r["alive"] = rng.integers(0, 1 << 32, len(r))
    quiet = rng.random(len(r)) < 0.1                                  # alive-only rows
    for f_ in ("count", "err_count", "sum_ns", "sumsq_us", "max_ns"):
        r[f_][quiet] = 0
    return r


def _random_map(rng, mk, mg, share=0.7, block=None):
    m = np.full(mk, engine.NO_GROUP, dtype=np.uint32)
    pick = rng.random(mk) < share
    m[pick] = (np.arange(mk)[pick] // block) % mg if block else rng.integers(0, mg, int(pick.sum()))
    return m
