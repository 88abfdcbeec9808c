"""Plain references for what lies between a window's rows and its scores (TEST INFRASTRUCTURE): K3's node statistics and node
features, K4's SAGE layer.  numpy, float64 and exact integers, no GPU.  Plus boundary_trace(): the smallest graph that crosses
every boundary of K3 and K4 (node ranges, edge slices, gather batches, mean blocks, the eight-at-a-time block-sum loop).

node_stats_ref      the twelve st_sum words and the two st_max words per node, from the rows' integers: exact.
node_features_ref   the 32 columns of x0 from those integers in float64, rounded once to fp32.  Against an
                    implementation of the same formulas the two fp32 values differ by at most 1 ulp: both sides round a float64 value
                    whose log1p, sqrt and division are each within 1 fp64 ulp of the true one, so the two fp32 roundings can only fall on
                    the same or on adjacent fp32 values.
sage_layer_ref      the layer in float64 with no pinned order, and a forward-error bound for the fp32 pinned-order result."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from alaz_amd import replay
from tests.probe_weights import _ev

# the words of st_sum (alaz_amd/csrc/sg_device.h ST_*): out and in side interleaved
ST_OUT_DEG, ST_IN_DEG, ST_OUT_CNT, ST_IN_CNT, ST_OUT_ERR, ST_IN_ERR, ST_OUT_SUM, ST_IN_SUM, ST_OUT_SSQ, ST_IN_SSQ, ST_OUT_ALIVE, ST_IN_ALIVE = range(12)
SUM_WORDS, MAX_WORDS = 12, 2
F_IN, F_HID = 32, 64
NODE_POD, NODE_SERVICE = 1, 2                                         # include/servicegraph.h SG_NODE_*
MEAN_SLOTS, MEAN_BLOCK = 16, 512                                      # the pinned order of the neighbour mean
K3_RANGE = 3072                                                       # nodes per range of k3_in_part (sg_sizes.h K3_IN_NR)
U32 = 2.0 ** -24                                                      # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------
# K3: node statistics and features
# ------------------------------------------------------------------------------------------------
def node_stats_ref(rows: np.ndarray, n_nodes: int, u: np.ndarray, v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(st_sum [n_nodes][12], st_max [n_nodes][2]) as u64, from a window's rows and their endpoints' dense ids (probe_weights.dense_ids):
    every row adds 1, count, err_count, sum_ns, sumsq_us and alive to the out words of its source and the in words of its destination,
    and its max_ns to their maxima.  u64 arithmetic: exact."""
    s = np.zeros((n_nodes, SUM_WORDS), dtype=np.uint64)
    m = np.zeros((n_nodes, MAX_WORDS), dtype=np.uint64)
    one = np.ones(len(rows), dtype=np.uint64)
    for side, idx in ((0, np.asarray(u, dtype=np.int64)), (1, np.asarray(v, dtype=np.int64))):
        for word, a in ((ST_OUT_DEG, one), (ST_OUT_CNT, rows["count"]), (ST_OUT_ERR, rows["err_count"]), (ST_OUT_SUM, rows["sum_ns"]),
                        (ST_OUT_SSQ, rows["sumsq_us"]), (ST_OUT_ALIVE, rows["alive"])):
            np.add.at(s[:, word + side], idx, a.astype(np.uint64))
        np.maximum.at(m[:, side], idx, rows["max_ns"].astype(np.uint64))
    return s, m


def node_features_ref(stats: Tuple[np.ndarray, np.ndarray], kind: np.ndarray) -> np.ndarray:
    """x0 [n][32] fp32 from (st_sum, st_max) and the nodes' kinds (SG_NODE_POD / SG_NODE_SERVICE / 0 = outbound): DESIGN.md §4 in
    float64, one rounding to fp32.  Columns: 0/1 log1p(out / in degree), 2/3 log1p(events), 4/5 log1p(mean latency in ms), 6/7 error
    ratio, 8/9 log1p(max latency in ms), 10/11/12 pod / service / outbound, 13/14 log1p(latency deviation in ms), 15 the constant 1,
    16/17 log1p(open connections), 18..31 zero."""
    s, m = stats
    f8 = np.float64
    n = len(s)
    x = np.zeros((n, F_IN), dtype=f8)
    kind = np.asarray(kind)
    with np.errstate(divide="ignore", invalid="ignore"):
        for side in (0, 1):
            deg, cnt, err = s[:, ST_OUT_DEG + side].astype(f8), s[:, ST_OUT_CNT + side].astype(f8), s[:, ST_OUT_ERR + side].astype(f8)
            sm, sq, mx = s[:, ST_OUT_SUM + side].astype(f8), s[:, ST_OUT_SSQ + side].astype(f8), m[:, side].astype(f8)
            has = cnt > 0
            mean_us = np.where(has, (sm / 1000.0) / cnt, 0.0)
            var = np.where(has, sq / cnt - mean_us * mean_us, 0.0)
            std_us = np.where(var > 0.0, np.sqrt(np.maximum(var, 0.0)), 0.0)
            x[:, 0 + side] = np.log1p(deg)
            x[:, 2 + side] = np.log1p(cnt)
            x[:, 4 + side] = np.log1p(mean_us / 1000.0)
            x[:, 6 + side] = np.where(has, err / cnt, 0.0)
            x[:, 8 + side] = np.log1p(mx / 1e6)
            x[:, 13 + side] = np.log1p(std_us / 1000.0)
            x[:, 16 + side] = np.log1p(s[:, ST_OUT_ALIVE + side].astype(f8))
    x[:, 10] = kind == NODE_POD
    x[:, 11] = kind == NODE_SERVICE
    x[:, 12] = kind == 0
    x[:, 15] = 1.0
    return x.astype(np.float32)


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """how many fp32 values lie between a and b (0 = bit-equal up to the sign of zero); finite inputs"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def csr_of(u: np.ndarray, v: np.ndarray, n_nodes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rowptr, col) of rows in canonical order (ascending source, then destination)"""
    u = np.asarray(u, dtype=np.int64); v = np.asarray(v, dtype=np.int64)
    assert np.all((u[1:] > u[:-1]) | ((u[1:] == u[:-1]) & (v[1:] > v[:-1]))), "rows are not in canonical order"
    rowptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=n_nodes), out=rowptr[1:])
    return rowptr, v


# ------------------------------------------------------------------------------------------------
# K4: the SAGE layer
# ------------------------------------------------------------------------------------------------
def _gamma(n, u=U32):
    n = np.asarray(n, dtype=np.float64)
    return n * u / (1.0 - n * u)


def sage_layer_ref(h_in: np.ndarray, rowptr: np.ndarray, col: np.ndarray, Ws: np.ndarray, Wn: np.ndarray, b: np.ndarray):
    """(h_out, bound): h_out [n][64] = ReLU(b + h_in Ws + mean_{out-neighbours}(h_in) Wn) in float64, in whatever order numpy sums; bound
    [n][64] >= |fp32 pinned-order result - h_out|, element by element.

    Derivation (u = 2^-24, gamma_n = n u / (1 - n u); Higham, Accuracy and Stability of Numerical Algorithms, §3.1):
      mean  The pinned order adds a neighbour's element into one of 16 slot sums, the slot sums into a block sum, the block sums into
            the row's total, and divides once.  Whatever the order, an addend passes through at most deg - 1 additions and the
            division: at most deg roundings, so the fp32 mean is sum_i x_i (1 + theta_i) / deg with |theta_i| <= gamma_deg <= gamma_{deg+1}:
                |dmean_k| <= gamma_{deg+1} * sum_nbr |h_in[nbr][k]| / deg.
      acc   The dense part is a chain of 2F fused multiply-adds that starts at b_j (F self terms, then F mean terms): one rounding each,
            so the first term passes through 2F roundings and the fp32 result is b_j (1 + t_0) + sum_k a_k w_kj (1 + t_k) with
            |t| <= gamma_{2F} over the fp32 operands a = (h, fp32 mean).  With fp32 mean = mean + dmean:
                |dacc_j| <= gamma_{2F+1} * (|b_j| + sum_k |h_k| |Ws_kj| + sum_k |mean_k| |Wn_kj|) + sum_k |dmean_k| |Wn_kj|.
            (The cross term gamma_{2F} sum |dmean_k| |Wn_kj| is of second order; the step from gamma_{2F} to gamma_{2F+1} pays for it:
            every input here is >= 0 — features, and outputs of a ReLU — so sum |h_in[nbr][k]| / deg = |mean_k|, and
            2F (deg + 1) u < 1 for every degree below 2^16.)
      ReLU  max(x, 0) is 1-Lipschitz and exact: it does not enlarge the bound.
    The float64 reference's own error obeys the same two formulas with u = 2^-53 and is added: it is 2^-29 of the rest."""
    f8 = np.float64
    h = np.asarray(h_in, dtype=f8)
    Ws = np.asarray(Ws, dtype=f8); Wn = np.asarray(Wn, dtype=f8); b = np.asarray(b, dtype=f8)
    n, F = h.shape
    assert Ws.shape == (F, F_HID) and Wn.shape == (F, F_HID) and b.shape == (F_HID,) and len(rowptr) == n + 1
    deg = np.diff(rowptr).astype(np.int64)
    src = np.repeat(np.arange(n), deg)
    tot = np.zeros((n, F), dtype=f8); tot_abs = np.zeros((n, F), dtype=f8)
    nb = h[np.asarray(col, dtype=np.int64)]
    np.add.at(tot, src, nb)
    np.add.at(tot_abs, src, np.abs(nb))
    d = np.maximum(deg, 1).astype(f8)[:, None]
    mean, mean_abs = tot / d, tot_abs / d
    acc = b[None, :] + h @ Ws + mean @ Wn
    mag = np.abs(b)[None, :] + np.abs(h) @ np.abs(Ws) + np.abs(mean) @ np.abs(Wn)
    bound = 0.0
    for u in (U32, 2.0 ** -53):
        dmean = _gamma(deg + 1, u)[:, None] * mean_abs
        bound = bound + _gamma(2 * F + 1, u) * mag + dmean @ np.abs(Wn)
    return np.maximum(acc, 0.0), bound


def layer_weights(w: np.ndarray, l: int):
    """(Ws, Wn, b) of layer l from a blob (alaz_amd/weights.py layout)"""
    off = sum(2 * (F_IN if k == 0 else F_HID) * F_HID + F_HID for k in range(l))
    fi = F_IN if l == 0 else F_HID
    Ws = w[off:off + fi * F_HID].reshape(fi, F_HID); off += fi * F_HID
    Wn = w[off:off + fi * F_HID].reshape(fi, F_HID); off += fi * F_HID
    return Ws, Wn, w[off:off + F_HID]


def pinned_mean32(h: np.ndarray, nbr: np.ndarray) -> np.ndarray:
    """the fp32 mean of rows `nbr` of h in the pinned order: blocks of 512 neighbours; inside a block neighbour i goes to slot i % 16
    (ascending i), the slots are combined 0..15; block sums added in block order; one division"""
    h = np.asarray(h, dtype=np.float32)
    total = None
    for b0 in range(0, len(nbr), MEAN_BLOCK):
        blk = h[nbr[b0:b0 + MEAN_BLOCK]]
        part = np.zeros((MEAN_SLOTS, h.shape[1]), dtype=np.float32)
        for i in range(0, len(blk), MEAN_SLOTS):
            c = blk[i:i + MEAN_SLOTS]
            part[:len(c)] = part[:len(c)] + c
        t = part[0].copy()
        for s in range(1, MEAN_SLOTS):
            t = t + part[s]
        total = t if total is None else total + t
    return total / np.float32(len(nbr))


def plain_mean32(h: np.ndarray, nbr: np.ndarray) -> np.ndarray:
    """the fp32 mean of the same rows added left to right"""
    return np.cumsum(np.asarray(h, dtype=np.float32)[nbr], axis=0, dtype=np.float32)[-1] / np.float32(len(nbr))


# ------------------------------------------------------------------------------------------------
# the boundary trace
# ------------------------------------------------------------------------------------------------
#: out-degrees of the hand-built hub pods, one row each: the 16 slots, one 64-neighbour gather batch, two batches, the 512-neighbour
#: block, two and eight blocks and their successors, and ten blocks (the eight-at-a-time block-sum loop and its remainder)
BOUNDARY_DEGREES = (1, 15, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513, 1024, 1025, 4096, 4097, 4700)
BOUNDARY_PODS, BOUNDARY_SVCS = 3200, 3000                            # known nodes: pods 0..3199 (the hubs last), services 3200..6199
#: nodes next to the boundaries of k3_in_part's ranges that receive hand-placed in-edges (and N - 1, the highest raw outbound IP)
BOUNDARY_NODES = (K3_RANGE - 1, K3_RANGE, 2 * K3_RANGE - 1, 2 * K3_RANGE)
IN_ONLY, OUT_ONLY = K3_RANGE - 1, K3_RANGE + 1                        # a pod with in-edges only, a pod with out-edges only
MANY_IN = BOUNDARY_PODS + 100                                         # a service with in-edges from more than 1024 sources
TOP_RAW_IP = 0xF0000001                                               # the highest raw outbound IP: node N - 1
_SPREAD_SOURCES = (2, 1601, 3100)                                     # sources at the start, the middle and the end of the base pods' rows


def boundary_ip(node: int) -> int:
    """IP of a known node of the boundary trace"""
    return replay.POD_IP_BASE + node if node < BOUNDARY_PODS else replay.SVC_IP_BASE + node - BOUNDARY_PODS


def boundary_trace(raw_outbound: bool = True):
    """(topology, events, labels): a mixed-protocol trace on 3200 pods and 3000 services (plus labels and raw outbound IPs: N spans
    three ranges of 3072 nodes), whose last 17 pods are hubs with out-rows of the lengths in BOUNDARY_DEGREES.  Nodes 3071, 3072, 6143,
    6144 and N - 1 receive in-edges from sources at the start, the middle and the end of the CSR and from the longest hub row; pod 3071
    has in-edges only, pod 3073 out-edges only; service MANY_IN has in-edges from 1100 pods and every hub of 511 neighbours or more; 600 open-connection
    records.  About 49 k events, 28 k edges."""
    H = len(BOUNDARY_DEGREES)
    P = BOUNDARY_PODS - H
    topo = replay.make_topology(P, 9000, seed=0xB0DA, svcs=BOUNDARY_SVCS)
    base, labels = replay.make_events(topo, 30_000, seed=0xB0DB, mixed=True, with_raw_outbound=raw_outbound)
    if not raw_outbound:                                             # (non-HTTP requests to unknown IPs carry no label: raw-IP nodes too)
        known = np.concatenate([topo.pod_ips, topo.svc_ips])
        base = base[(np.isin(base["saddr"], known) & np.isin(base["daddr"], known)) | (base["host_label"] != 0)]
    base = base[(base["saddr"] != boundary_ip(IN_ONLY)) & (base["daddr"] != boundary_ip(OUT_ONLY))]
    hub_ips = (replay.POD_IP_BASE + P + np.arange(H)).astype(np.uint32)
    rng = np.random.default_rng(0xB0DC)
    parts = [base]
    # in-edges at the range boundaries, from sources whose rows lie far apart in the CSR
    spread = np.array([boundary_ip(s) for s in _SPREAD_SOURCES], dtype=np.uint32)
    targets = [boundary_ip(b) for b in BOUNDARY_NODES] + ([TOP_RAW_IP] if raw_outbound else [])
    for i, t in enumerate(targets):
        parts.append(_ev(3, spread, t, np.array([3_000_000, 40_000_000, 700_000], dtype=np.uint64) + np.uint64(1000 * i)))
    parts.append(_ev(2, boundary_ip(OUT_ONLY), np.array([boundary_ip(BOUNDARY_PODS + 7), boundary_ip(5)], dtype=np.uint32), 2_500_000))
    # one destination with more than 1024 sources, spread over the base pods' rows
    many = (replay.POD_IP_BASE + 1 + 2 * np.arange(1100)).astype(np.uint32)
    parts.append(_ev(len(many), many, boundary_ip(MANY_IN), np.rint(np.exp(np.log(5e6) + 0.8 * rng.standard_normal(len(many)))).astype(np.uint64)))
    # the hub rows: the longest one reaches every boundary node and MANY_IN
    cand = np.concatenate([topo.svc_ips, topo.pod_ips])
    forced = np.array(targets + [boundary_ip(MANY_IN)], dtype=np.uint32)
    cand = cand[~np.isin(cand, forced) & (cand != boundary_ip(OUT_ONLY))]
    for h, deg in enumerate(BOUNDARY_DEGREES):
        dst = cand[rng.permutation(len(cand))[:deg]]
        if deg == max(BOUNDARY_DEGREES):                             # (the last hub: its row ends the CSR)
            dst[:len(forced)] = forced
        elif deg >= 511:                                             # MANY_IN's in-edges: in every part of the CSR
            dst[0] = boundary_ip(MANY_IN)
        dur = np.rint(np.exp(np.log(5e6) + 0.5 * rng.standard_normal(deg))).astype(np.uint64)
        parts.append(_ev(deg, hub_ips[h], dst, dur))
    # open connections: busy pairs, idle pairs and (raw_outbound) raw IPs never seen otherwise
    al = np.zeros(600, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    src = rng.integers(0, P, len(al)); src[src == IN_ONLY] = 0
    dpod = rng.integers(0, P, len(al)); dpod[dpod == OUT_ONLY] = 1
    al["saddr"] = topo.pod_ips[src]
    pick = rng.random(len(al))
    far = 0x5DB8D800 + rng.integers(0, 30, len(al)) if raw_outbound else topo.pod_ips[dpod]
    al["daddr"] = np.where(pick < 0.6, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))], np.where(pick < 0.85, topo.pod_ips[dpod], far)).astype(np.uint32)
    parts.append(al)
    ev = np.concatenate(parts)
    ext = replay.Topology(P + H, topo.n_svcs, np.concatenate([topo.pod_ips, hub_ips]), topo.svc_ips, topo.edge_src, topo.edge_dst, topo.seed)
    return ext, ev, labels


def sparse_trace(n_pods: int, hot_from: int, n_events: int, seed: int, n_svcs: int = 64):
    """(topology, events, labels) on n_pods pods of which only a few hundred speak: half of the events run between pods and services
    with ids from hot_from upwards (a kernel's second trip over the nodes), half between the first 200 pods and those; no labels"""
    pod_ips = (replay.POD_IP_BASE + np.arange(n_pods, dtype=np.uint64)).astype(np.uint32)
    svc_ips = (replay.SVC_IP_BASE + np.arange(n_svcs, dtype=np.uint64)).astype(np.uint32)
    topo = replay.Topology(n_pods, n_svcs, pod_ips, svc_ips, np.zeros(0, np.int64), np.zeros(0, np.int64), seed)
    rng = np.random.default_rng(seed)
    hot = np.arange(hot_from, n_pods)
    low = np.arange(200)
    src = np.where(rng.random(n_events) < 0.5, rng.choice(hot, n_events), rng.choice(low, n_events))
    to_svc = (rng.random(n_events) < 0.4) & (n_svcs > 0)
    dpod = np.where(rng.random(n_events) < 0.6, rng.choice(hot, n_events), rng.choice(low, n_events))
    dpod = np.where(dpod == src, (dpod + 1) % n_pods, dpod)
    ev = _ev(n_events, pod_ips[src], np.where(to_svc, svc_ips[rng.integers(0, max(n_svcs, 1), n_events) % max(n_svcs, 1)] if n_svcs else 0, pod_ips[dpod]).astype(np.uint32),
             np.rint(np.exp(np.log(5e6) + 0.8 * rng.standard_normal(n_events))).astype(np.uint64))
    ev["status"] = np.where(rng.random(n_events) < 0.05, 503, 200).astype(np.uint16)
    return topo, ev, []


# ------------------------------------------------------------------------------------------------
# the oracle's window of a trace, closed once per process
# ------------------------------------------------------------------------------------------------
_WINDOWS = {}


def oracle_window(key, trace, layers: int, clock) -> dict:
    """the C oracle's window of trace() = (topology, events, labels) under make_weights(layers), cached under (key, layers): n, rows,
    dense ids u / v, the nodes' kinds, the blob w, stats = (st_sum, st_max), x0 and h[1..layers]"""
    if (key, layers) not in _WINDOWS:
        from alaz_amd import weights
        from oracle import pyoracle
        from tests.probe_weights import dense_ids
        topo, ev, labels = trace()
        o = pyoracle.Oracle(*clock)
        o.apply_ops(topo.k8s_ops()); o.packed(ev, labels)
        w = weights.make_weights(layers)
        o.window_close(w, layers)
        rows = o.edge_rows()
        u, v = dense_ids(o, rows)
        assert o.n_known == topo.n_nodes
        kind = np.zeros(o.n_nodes, dtype=np.uint8)
        kind[:topo.n_pods] = NODE_POD; kind[topo.n_pods:topo.n_nodes] = NODE_SERVICE
        _WINDOWS[(key, layers)] = dict(n=o.n_nodes, rows=rows, u=u, v=v, kind=kind, w=w, stats=o.node_stats(), x0=o.node_features(),
                                       h=[None] + [o.layer_output(l) for l in range(1, layers + 1)])
        o.close()
    return _WINDOWS[(key, layers)]
