"""What the GPU tests of the window stages (K8 - K23) share: the engines they build, how they feed them and read device memory, the
workload maps and the constructed windows.  Not a test module: nothing here is collected, and asserts carry their own messages
(pytest rewrites asserts in test modules only).  The traces are in tests/traces.py; K1 - K5's scaffolding in tests/gpu_model_scaffold.py."""
import ctypes

import numpy as np
import pytest

from alaz_amd import engine, replay, weights
from tests.helpers import CLOCK, HostShim
from tests.incident_ref import incident_ref

ME = 1 << 15
INF = float("inf")
PARAMS = dict(shift=3, warmup=2, ttl=3, max_entries=700)       # a small ttl, and a capacity the churn overflows


def _engine(topo, labels, layers=2, *, variant=0, max_edges=ME, max_obip=512, **kw):
    if variant == 0:                                                  # the 8-byte-record path with the warm state kept
        kw.setdefault("warm", True)
        variant = 3
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=256,
                            max_outbound_ips=max_obip, k1_variant=variant, max_window_events=kw.pop("max_window_events", 300_000),
                            max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(layers))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


# K8's engine (tests/test_gpu_trend.py and the two that follow it import it as _engine): max_outbound_ips is fixed
def _trend_engine(topo, labels, layers=2, *, variant=0, max_edges=ME, **kw):
    if variant == 0:                                                  # the 8-byte-record path with the warm state kept
        kw.setdefault("warm", True)
        variant = 3
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=max_edges, layers=layers, max_labels=256,
                            max_outbound_ips=512, k1_variant=variant, max_window_events=kw.pop("max_window_events", 300_000),
                            max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(layers))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def _ncap(g):
    return g.window_buffers()[3]                                      # the node capacity (sg_window_buffers)


def _feed(g, ev):
    if len(ev):
        g.ingest_bulk(np.ascontiguousarray(ev))


def _rc(call, *a, **kw):
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(*a, **kw)
    return ei.value.rc


def _path(before, after):
    d = {k: getattr(after, k) - getattr(before, k) for k in ("windows_cold", "windows_warm", "windows_delta", "windows_plain")}
    if d["windows_delta"]:
        return "delta"
    return "warm" if d["windows_warm"] else "cold" if d["windows_cold"] else "plain" if d["windows_plain"] else "none"


def _hip():
    hip = ctypes.CDLL(None)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def _d2h(hip, ptr, n, dtype):
    out = np.zeros(n, dtype=dtype)
    if n:
        rc = hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, 2)
        assert rc == 0, ("hipMemcpy to the host", rc, hex(ptr), out.nbytes)
    return out


def _map(kind, mk, n_pods):
    m = np.full(mk, engine.NO_GROUP, np.uint32)
    if kind == "blocks":
        m[:n_pods] = np.arange(n_pods) // 7
    elif kind == "one":
        m[:n_pods] = 0
    return m


def _grouped(topo, labels, kind, **kw):
    g = _engine(topo, labels, **kw)
    mk = topo.n_nodes + 8
    gmap = _map(kind, mk, topo.n_pods)
    g.set_groups()
    g.group_assign(np.arange(mk), gmap)
    return g, gmap, mk


N_PODS = 150                                                          # 22 350 ordered pairs: windows of up to 3 tiles + 1 rows


def _pods_engine(max_known=None, max_groups=0, n_pods=N_PODS, **kw):
    topo = replay.make_topology(n_pods, 4 * n_pods, seed=7, svcs=4)    # (only the pods and their ids are used)
    mk = max_known or topo.n_nodes + 8
    g = engine.ServiceGraph(max_known_nodes=mk, max_edges=1 << 14, layers=2, max_labels=kw.pop("max_labels", 16),
                            max_outbound_ips=kw.pop("max_outbound_ips", 64), max_window_events=1 << 16, max_batch=1 << 14, **kw)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    return topo, g, mk


def _pairs(n_pods, E, seed):
    """E distinct (src, dst) pairs, src != dst, from a seeded permutation of all of them"""
    allp = np.array([(i, j) for i in range(n_pods) for j in range(n_pods) if i != j])
    p = allp[np.random.default_rng(seed).permutation(len(allp))[:E]]
    return p[:, 0], p[:, 1]


EXT = 0x5DB8D800                                                      # addresses outside the cluster


def _events(topo, src, daddr, dur=1_000_000, alive=None, status=None, label=None):
    """one request (or, where alive, one alive record) per (src pod, destination address) pair"""
    src = np.asarray(src, dtype=np.int64)
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = daddr
    e["status"] = 200 if status is None else status
    e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = dur
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    if label is not None:
        e["host_label"] = label
    if alive is not None:
        a = np.asarray(alive, bool)
        e["flags"][a] = replay.EV_ALIVE
        e["status"][a] = 0; e["protocol"][a] = 0; e["duration_ns"][a] = 0
    return e


def _send(topo, g, src, dst, **kw):
    e = _events(topo, src, topo.pod_ips[np.asarray(dst, dtype=np.int64)], **kw)
    if len(e):
        g.ingest_bulk(e)
    return g.flush_window().copy()


# (rows in front of the long run, its length): a run inside a span of K9_ROWS = 8, cut by spans, ending on an end of a chunk of
# K9_CHUNK = 2048 (8 + 2040, 6 + 2042), crossing one, beginning at one (2048 in front), and passing THROUGH a whole chunk (6 + 4097
# covers [2048, 4096)).  tests/test_gpu_group_nodes.py holds K16's out side to the same list.
RUNS = [(6, 1), (6, 7), (6, 8), (6, 9), (6, 2047), (6, 2048), (6, 2049), (6, 4097), (8, 2040), (6, 2042), (2048, 9), (2047, 2049), (5, 3)]


# ---- K12's constructed windows (tests/test_gpu_incidents.py, tests/test_gpu_tracks.py): pod-to-pod events only and min_value = -inf,
# so every row is red.  The workload stages' _pods_engine above is another engine: no stage is on, and it returns max_known too.



def _check_incidents(g, rows, by="score", thr=0.0, nodes=None, got=None, ginc=None):
    """the last read window's incidents (or `got`, `ginc`) against the reference over `rows`, the window's node rows and — where the
    engine has them — its trend and rank rows"""
    nodes = g.window_nodes() if nodes is None else nodes
    trend = g.window_trend() if by != "score" else None
    try:
        rank = g.window_rank()
    except engine.ServiceGraphError:
        rank = None                                                   # the ranking is off
    want, winc = incident_ref(rows, nodes, by, thr, trend=trend, rank=rank)
    got = g.window_incidents() if got is None else got
    ginc = g.window_node_incident() if ginc is None else ginc
    assert len(got) == len(want), (len(got), len(want), by, thr)
    assert got.tobytes() == want.tobytes(), (by, thr)
    assert ginc.tobytes() == winc.tobytes(), ("the incident of each node row", by, thr, ginc[:8].tolist(), winc[:8].tolist())
    assert (got["culprit_node"] == engine.NO_INCIDENT).all() == (rank is None or len(got) == 0), ("culprits without a ranking", got["culprit_node"][:8].tolist(), rank is None)
    return got


def _incident_pods_engine(n_pods, max_known=None, max_edges=1 << 14):
    topo = replay.make_topology(n_pods, 4 * n_pods, seed=7, svcs=4)    # (only the pods and their ids are used)
    g = engine.ServiceGraph(max_known_nodes=max_known or topo.n_nodes + 8, max_edges=max_edges, layers=2, max_labels=16, max_outbound_ips=64,
                            max_window_events=1 << 16, max_batch=1 << 14)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(2))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(0)
    g.set_nodes(); g.set_rank(iters=2); g.set_incidents(min_value=-INF)
    return topo, g


def _incident_close(topo, g, src, dst):
    """one request per (src pod, dst pod) pair; the window's rows, its incidents and the incident per node row (checked against
    the reference); pod i has node id i, so its KNOWN ref is i and the node rows are ascending in pod id"""
    src, dst = np.asarray(src), np.asarray(dst)
    e = np.zeros(len(src), dtype=replay.EVENT_DTYPE)
    e["saddr"] = topo.pod_ips[src]; e["daddr"] = topo.pod_ips[dst]; e["status"] = np.where(np.arange(len(e)) % 3 == 0, 503, 200)
    e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = 1_000_000 + 37 * np.arange(len(e), dtype=np.uint64)
    e["write_time_ns"] = np.uint64(2_000_000_000) + np.uint64(100) * np.arange(len(e), dtype=np.uint64)
    g.ingest_bulk(e)
    rows = g.flush_window().copy()
    assert len(rows) == len(e) and sorted(zip(rows["from_ref"].tolist(), rows["to_ref"].tolist())) == sorted(zip(src.tolist(), dst.tolist())), \
        ("one row per (src, dst) pair", len(rows), len(e))
    nodes = g.window_nodes()
    got = _check_incidents(g, rows, "score", -INF, nodes)
    return rows, nodes, got, g.window_node_incident()
