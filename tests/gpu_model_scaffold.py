"""What the GPU tests of pass A, the model stages and the score kernel (K1 - K5) share: their traces and the oracle's windows of them
(made once per process), device reads and writes, the development build's knobs and the checks against the references.  Not a test
module: nothing here is collected, and asserts carry their own messages (pytest rewrites asserts in test modules only)."""
import contextlib
import ctypes
import os

import numpy as np

from alaz_amd import replay, weights
from tests import model_ref as mr
from tests import probe_weights as pw
from tests.helpers import CLOCK, compare_edge_dicts, engine_edge_dict

C_N_NODES, C_COUNT = 10, 40                                          # alaz_amd/csrc/sg_device.h
SCORE_BAR = 1e-5
INT_FIELDS = ("from_ref", "to_ref", "count", "err_count", "sum_ns", "max_ns", "sumsq_us", "alive")


def _boundary_half():
    topo, ev, labels = mr.boundary_trace()
    return topo, ev[::2].copy(), labels


#: name -> (trace, max_edges of its engines)
TRACES = {
    "adversarial": (pw.adversarial_trace, 16384),
    "boundary": (mr.boundary_trace, 32768),
    "boundary_known": (lambda: mr.boundary_trace(False), 32768),      # no raw outbound IPs: every window after the first may close warm
    "boundary_half": (_boundary_half, 32768),
    "sparse33k": (lambda: mr.sparse_trace(33_000, 32_700, 6000, seed=0x5A33), 8192),
}
_TRACE = {}


def trace(name):
    if name not in _TRACE:
        _TRACE[name] = TRACES[name][0]()
    return _TRACE[name]


def oracle(name, layers):
    """the oracle's window of the trace (closed once per process) with the float64 references of its statistics and features"""
    o = mr.oracle_window(name, lambda: trace(name), layers, CLOCK)
    if "ref_stats" not in o:
        o["ref_stats"] = mr.node_stats_ref(o["rows"], o["n"], o["u"], o["v"])
        o["ref_x0"] = mr.node_features_ref(o["ref_stats"], o["kind"])
        o["csr"] = mr.csr_of(o["u"], o["v"], o["n"])
    return o


# ---- device memory ----------------------------------------------------------------------------------------------------------------
_HIP = []


def _hip():
    if not _HIP:
        import torch  # noqa: F401  (the HIP runtime the engine shares)
        hip = ctypes.CDLL(None)
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipMemcpy.restype = ctypes.c_int
        _HIP.append(hip)
    return _HIP[0]


def _sync():
    import torch
    torch.cuda.synchronize()


def dev_read(ptr, shape, dtype):
    _sync()
    buf = np.empty(shape, dtype=dtype)
    rc = _hip().hipMemcpy(buf.ctypes.data, ctypes.c_void_p(ptr), buf.nbytes, 2)
    assert rc == 0, ("hipMemcpy to the host", rc, hex(ptr), buf.nbytes)
    return buf


def dev_write(ptr, arr):
    _sync()
    a = np.ascontiguousarray(arr)
    rc = _hip().hipMemcpy(ctypes.c_void_p(ptr), a.ctypes.data, a.nbytes, 1)
    assert rc == 0, ("hipMemcpy to the device", rc, hex(ptr), a.nbytes)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@contextlib.contextmanager
def knobs(**kv):
    """SG_* knobs of the development build, set while its engines are created"""
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in kv:
            os.environ.pop(k, None)


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def check_rows(rows, want, tag):
    assert len(rows) == len(want), tag
    for f in INT_FIELDS:
        assert np.array_equal(rows[f], want[f]), (tag, f)
    d = np.abs(rows["score"].astype(np.float64) - want["score"])
    assert d.max() <= SCORE_BAR, (tag, float(d.max()), int(np.argmax(d)))


def check_stats(E, o, tag):
    N = o["n"]
    assert E.n_nodes() == N, tag
    s, m = E.stats()
    for ref_s, ref_m in (o["stats"], o["ref_stats"]):
        bad = np.argwhere(s[:N] != ref_s)
        assert len(bad) == 0, (tag, "st_sum", bad[:4].tolist(), s[:N][tuple(bad[0])], ref_s[tuple(bad[0])])
        bad = np.argwhere(m[:N] != ref_m)
        assert len(bad) == 0, (tag, "st_max", bad[:4].tolist())
    assert not s[N:].any() and not m[N:].any(), (tag, "statistics beyond the window's nodes")


def check_x0(x0, o, tag):
    """x0[:N] within 1 ulp of the oracle's and of the float64 reference; -> is it bit-equal to the oracle's everywhere"""
    assert np.isfinite(x0).all(), tag
    counts = []
    for what, ref in (("the oracle", o["x0"]), ("the float64 reference", o["ref_x0"])):
        d = mr.ulp_distance(x0, ref)
        counts.append(int((d != 0).sum()))
        print(f"{tag}: {counts[-1]} of {d.size} elements of x0 are not bit-equal to {what} (max {int(d.max())} ulp)")
        assert d.max() <= 1, (tag, what, int(d.max()), np.argwhere(d > 1)[:4].tolist())
    assert np.all(bits(x0[:, 18:]) == 0) and np.all(x0[:, 15] == 1.0), tag
    return counts[0] == 0 and np.array_equal(bits(x0), bits(o["x0"]))


# ---- pass A's and the score kernel's trace (tests/test_gpu_pair_tiles.py, test_gpu_k5_forms.py and those that follow them) --------
MAX_LABELS = 64
STATS = ("last_window_events", "last_window_edges", "last_window_nodes", "last_window_tmin_ms", "last_window_tmax_ms", "events_dropped_src",
         "events_dropped_cap", "events_dropped_ring", "events_misrouted", "alive_in", "alive_dropped")
_CACHE = {}


def _topo():
    if "topo" not in _CACHE:
        topo = replay.make_topology(2000, 36_000, seed=231)
        # one IP in both maps: a service with pod 1's address (the service wins as destination, data.go:840-849)
        ops = topo.k8s_ops() + [("svc", "ADD", "svc-shadowing-pod1", replay.ip_str(int(topo.pod_ips[1])))]
        ev, labels = replay.make_events(topo, 160_000, 232, mixed=True, with_raw_outbound=True, with_reverse=True)
        assert len(labels) <= MAX_LABELS, (len(labels), MAX_LABELS)
        known = np.isin(ev["daddr"], np.concatenate([topo.pod_ips, topo.svc_ips])) & (ev["daddr"] != topo.pod_ips[1])
        plain = ev[known & (ev["duration_ns"] < (1 << 32)) & ((ev["flags"] & replay.EV_ALIVE) == 0)]
        assert len(plain) > 100_000, len(plain)
        _CACHE["topo"] = (topo, ops, ev, plain, labels)
    return _CACHE["topo"]


def _sorted(rows):
    return rows[np.lexsort((rows["to_ref"], rows["from_ref"]))]


def _on_edges(e, rng):
    """one plain request per entry of e, on that topology edge"""
    topo, _, _, plain, _ = _topo()
    ev = np.repeat(plain[:1], len(e))
    ev["flags"] = 0; ev["host_label"] = 0
    ev["saddr"] = topo.pod_ips[topo.edge_src[e]]; ev["daddr"] = topo.node_ip(topo.edge_dst[e])
    ev["duration_ns"] = rng.integers(1, 1 << 30, len(e)); ev["status"] = np.where(rng.random(len(e)) < 0.1, 503, 200)
    return ev


_ORACLE = {}


def _feed(g, ev):
    if len(ev):
        while g.ingest(ev) != 0:
            pass


def _close(g, how, layers):
    if how == "flush":
        return g.flush_window().copy()
    if how == "run":                                                 # the one-call pipeline: k5_edge_score<RESET = true>
        g.window_run()
        return g.window_read().copy()
    g.window_close(); g.window_features()                            # the staged calls: RESET = false, sg_window_reset behind them
    for l in range(layers):
        g.window_layer(l)
    g.window_score()
    rows = g.window_read().copy()
    g.window_reset()
    return rows


def _mixed(lo=0, hi=65536):
    """the mixed trace of test_gpu_pair_tiles (Host labels, raw outbound IPs, reversed events), every 53rd event an open connection
    from a pod"""
    if ("mixed", lo, hi) not in _ORACLE:
        topo, _, ev, _, _ = _topo()
        ev = ev[lo:hi].copy()
        at = np.arange(7, len(ev), 53)
        ev["flags"][at] = replay.EV_ALIVE
        ev["saddr"][at] = topo.pod_ips[topo.edge_src[at % len(topo.edge_src)]]
        _ORACLE[("mixed", lo, hi)] = ev
    return _ORACLE[("mixed", lo, hi)]


def _oracle_windows(key, windows, layers):
    if key not in _ORACLE:
        from oracle import pyoracle
        _, ops, _, _, labels = _topo()
        o = pyoracle.Oracle(*CLOCK); o.apply_ops(ops)
        W = weights.make_weights(layers)
        res = []
        for ev in windows:
            o.packed(ev, labels); o.window_close(W, layers)
            res.append((o.edge_dict(), o.edge_rows().copy()))
        _ORACLE[key] = res
    return _ORACLE[key]


def _check_oracle(res, shim, ref):
    labels = _topo()[4]
    for (rows, _, ob), (edict, orow) in zip(res, ref):
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, ob), edict)
        assert np.array_equal(rows["from_ref"], orow["from_ref"]) and np.array_equal(rows["to_ref"], orow["to_ref"]), \
            ("the rows' order against the oracle's", len(rows), len(orow))
