"""Probe weight blobs: blobs under which an edge's score reads out ONE internal quantity of the model (TEST INFRASTRUCTURE).

The default blob (alaz_amd.weights.make_weights) keeps every score near 0.5 and every logit within about +-0.3, so the 1e-5 score bar
of the parity tests lets through feature errors of hundreds of fp32 ulps.  A probe blob routes one quantity phi per edge through
one-hot weights into hidden unit 0 of the score head, with w2[0] = -1 and everything else zero, so that

    logit = -(c * phi + off),    phi = log((1 - s) / s) / c - off / c      (s = the row's score, taken to float64)

c is a power of two and phi is an fp32 value, so c * phi is exact, every other term on the route is an exact zero and (off = 0)
the logit is exact on both sides.  The only roundings are in the sigmoid: expf (within 1 ulp on the device and in libm), the
addition of 1 and the division (0.5 ulp each), so the score carries a relative error of at most 2 eps (eps = 2^-23, a generous ulp).
For logit <= 0, d log((1 - s) / s) / ds * s = -1 / (1 - s), at most 2 in size, so the recovered c * phi is off by at most 4 eps =
2^-21 from the true one, on either side.  Two readouts of the same phi (the engine's, the oracle's) therefore differ by at most
READOUT_BOUND / c = 2^-20 / c (1.2e-7 at c = 8); one readout lies within half of that of phi itself.  test_probe_weights measures
the oracle's readouts against its own features: they stay inside the half bound (measured: 2.9e-8 at c = 8, 3.8e-8 at c = 4).

Layout of the blob: alaz_amd/weights.py.  Signed quantities (the clamped z of e6, in [-1, 1]) are lifted by off = c through b1[0]
so the logit stays <= 0; off + c * phi is then one fp32 rounding (an fma), the same on both sides, which expected() applies to
the float64 reference too."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from alaz_amd import replay
from alaz_amd.weights import F_EDGE, F_HID, layer_in, weights_count

#: the bound on |phi_a - phi_b| * c between two readouts of the same fp32 phi (module docstring: 2 x 4 eps, eps = 2^-23)
READOUT_BOUND = 2.0 ** -20
#: the non-constant columns of a node's feature vector x (sg_k3.h k3_node_features): 15 is the constant 1, 18..31 are zero
NODE_COLUMNS = tuple(range(15)) + (16, 17)


def offsets(layers: int) -> Dict[str, int]:
    """float offsets of every tensor in the blob (alaz_amd/weights.py layout)"""
    o, off = {}, 0
    for l in range(layers):
        fi = layer_in(l)
        o[f"Ws{l}"] = off; off += fi * F_HID
        o[f"Wn{l}"] = off; off += fi * F_HID
        o[f"b{l}"] = off; off += F_HID
    for name, n in (("Wu", F_HID * F_HID), ("Wv", F_HID * F_HID), ("We", F_EDGE * F_HID), ("b1", F_HID), ("w2", F_HID), ("b2", 1)):
        o[name] = off; off += n
    assert off == weights_count(layers)
    return o


@dataclass(frozen=True)
class Probe:
    name: str
    kind: str          # "src" / "dst" (a node feature of the edge's endpoint), "mean" / "mean2" / "selfmean" (layer outputs), "edge", "const"
    col: int           # the column of x (node kinds, mean kinds) or of the edge features (edge)
    c: float           # readout scale (a power of two)
    off: float         # logit offset (edge e6 only)
    w: np.ndarray      # the blob

    def bound(self) -> float:
        return READOUT_BOUND / self.c


def _blob(layers: int, **set_) -> np.ndarray:
    w = np.zeros(weights_count(layers), dtype=np.float32)
    o = offsets(layers)
    for key, val in set_.items():
        name, idx = key.split("__")
        w[o[name] + int(idx)] = np.float32(val)
    w[o["w2"]] = -1.0
    return w


# columns whose values can exceed 10 on the adversarial trace (log1p of event counts of 1e4 and more; log1p of a mean, std or max
# in ms, up to 1e6 ms): c = 4 keeps c * phi below 87, where the score would leave the normal fp32 range
_WIDE_NODE = {2, 3, 4, 5, 8, 9, 13, 14}
_WIDE_EDGE = {1, 2, 3}


def probes(layers: int) -> List[Probe]:
    """every probe of a model with `layers` SAGE layers"""
    out: List[Probe] = []
    hop = {"Ws1__0": 1.0} if layers == 2 else {}                     # layer 1 passes unit 0 of layer 0 on (self term)
    for col in NODE_COLUMNS:
        c = 4.0 if col in _WIDE_NODE else 8.0
        for side, head in (("src", "Wu__0"), ("dst", "Wv__0")):
            out.append(Probe(f"{side}_x{col}", side, col, c, 0.0, _blob(layers, **{f"Ws0__{col * F_HID}": c, **hop, head: 1.0})))
        out.append(Probe(f"mean_x{col}", "mean", col, c, 0.0, _blob(layers, **{f"Wn0__{col * F_HID}": c, **hop, "Wu__0": 1.0})))
        if layers == 2:
            out.append(Probe(f"mean2_x{col}", "mean2", col, c, 0.0, _blob(layers, **{f"Wn0__{col * F_HID}": c, "Wn1__0": 1.0, "Wu__0": 1.0})))
            out.append(Probe(f"selfmean_x{col}", "selfmean", col, c, 0.0, _blob(layers, **{f"Ws0__{col * F_HID}": c, "Wn1__0": 1.0, "Wu__0": 1.0})))
    for k in range(F_EDGE):
        c = 4.0 if k in _WIDE_EDGE else 8.0
        off = c if k == 6 else 0.0                                   # e6 = clamp(z) / 8 lies in [-1, 1]
        out.append(Probe(f"edge_e{k}", "edge", k, c, off, _blob(layers, **{f"We__{k * F_HID}": c, "b1__0": off})))
    out.append(Probe("const_b2", "const", 0, 1.0, 0.0, _blob(layers, b2__0=-0.71875)))
    z = np.zeros(weights_count(layers), dtype=np.float32)
    out.append(Probe("zero", "const", 0, 1.0, 0.0, z))
    return out


def mean_probes(layers: int) -> List[Probe]:
    return [p for p in probes(layers) if p.kind in ("mean", "mean2", "selfmean")]


def readout(p: Probe, score: np.ndarray) -> np.ndarray:
    """phi per row from the rows' fp32 scores"""
    s = np.asarray(score, dtype=np.float64)
    assert np.all((s > 0.0) & (s < 1.0)), "a probe's score saturated: its c is too large for the trace"
    return (np.log1p(-s) - np.log(s)) / p.c - p.off / p.c


def expected(p: Probe, phi32: np.ndarray) -> np.ndarray:
    """what readout() returns for an exact sigmoid, given the fp32 quantity phi: the lift of e6 rounds once in fp32"""
    if p.off == 0.0:
        return phi32.astype(np.float64)
    t = (np.float32(p.c) * phi32.astype(np.float32)).astype(np.float64) + p.off      # fma(e, c, off): one rounding of the exact sum
    return t.astype(np.float32).astype(np.float64) / p.c - p.off / p.c


# ------------------------------------------------------------------------------------------------
# what a probe reads, from the oracle's own arrays
# ------------------------------------------------------------------------------------------------
def dense_ids(o, rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """canonical node ids of the rows' endpoints (known ids, then labels, then raw outbound IPs by rank)"""
    nk, nl = o.n_known, len(o.labels)
    nob = len(o.outbound_ips())
    assert o.n_nodes == nk + nl + nob

    def dense(ref):
        t, v = ref >> 30, (ref & 0x3FFFFFFF).astype(np.int64)
        return np.where(t == 0, v, np.where(t == 1, nk + v, nk + nl + v))
    return dense(rows["from_ref"]), dense(rows["to_ref"])


def oracle_phi(p: Probe, o, rows: np.ndarray) -> np.ndarray:
    """the fp32 quantity the probe reads, per row, from the oracle's features and layer outputs (its last closed window)"""
    u, v = dense_ids(o, rows)
    if p.kind in ("src", "dst"):
        x = o.node_features()[:, p.col]
        return x[u] if p.kind == "src" else x[v]
    if p.kind in ("mean", "mean2", "selfmean"):
        h = o.layer_output(1 if p.kind == "mean" else 2)[:, 0]        # (at L = 2 Ws1 = 1 passes the one-hop mean on: h2 = h1 there)
        return (h / np.float32(p.c))[u]
    if p.kind == "edge":
        return edge_features_ref(rows)[:, p.col]
    return np.full(len(rows), np.nan, np.float32)


def edge_features_ref(rows: np.ndarray) -> np.ndarray:
    """the eight edge features per row, restated in float64 from the rows' own integers and rounded to fp32:
    log1p(count), log1p(mean_ms), log1p(std_ms), log1p(max_ms), err / count, log1p(err), clamp(z, -8, 8) / 8, 1.  z compares the
    edge's mean with its source's: mean and std over the sums of the integers of every row with the same source."""
    f8 = np.float64
    cnt = rows["count"].astype(f8); err = rows["err_count"].astype(f8)
    sm = rows["sum_ns"].astype(f8); ssq = rows["sumsq_us"].astype(f8); mx = rows["max_ns"].astype(f8)

    def mean_std(s, q, c):
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(c > 0, (s / 1000.0) / c, 0.0)
            var = np.where(c > 0, q / c - m * m, 0.0)
        return m, np.where(var > 0.0, np.sqrt(np.maximum(var, 0.0)), 0.0)
    m_e, s_e = mean_std(sm, ssq, cnt)
    src = rows["from_ref"]
    _, inv = np.unique(src, return_inverse=True)
    # u64 sums of the integers per source (exact), then to float64 as the oracle does
    def usum(a):
        acc = np.zeros(inv.max() + 1 if len(inv) else 0, dtype=np.uint64)
        np.add.at(acc, inv, a.astype(np.uint64))
        return acc[inv].astype(f8)
    mu, sd = mean_std(usum(rows["sum_ns"]), usum(rows["sumsq_us"]), usum(rows["count"]))
    z = (m_e - mu) / np.where(sd > 1.0, sd, 1.0)
    zc = np.clip(z.astype(np.float32), np.float32(-8.0), np.float32(8.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        er = np.where(cnt > 0, err / np.maximum(cnt, 1.0), 0.0)
    e = np.stack([np.log1p(cnt), np.log1p(m_e / 1000.0), np.log1p(s_e / 1000.0), np.log1p(mx / 1e6), er, np.log1p(err),
                  np.zeros_like(cnt), np.ones_like(cnt)], axis=1).astype(np.float32)
    e[:, 6] = zc * np.float32(0.125)
    return e


def ulp32(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------------
# the adversarial trace
# ------------------------------------------------------------------------------------------------
#: out-degrees of the hand-built hub pods: one row of each of these lengths (K4's 16 interleaved slots and 512-neighbour blocks)
HUB_DEGREES = (1100, 513, 512, 511, 17, 16, 15, 1)


def _ev(n, saddr, daddr, dur, status=200, t0=2_000_000_000):
    e = np.zeros(n, dtype=replay.EVENT_DTYPE)
    e["saddr"] = saddr; e["daddr"] = daddr; e["status"] = status; e["protocol"] = replay.PROTO_HTTP
    e["duration_ns"] = dur
    e["write_time_ns"] = np.uint64(t0) + np.arange(n, dtype=np.uint64) * np.uint64(100)
    return e


def adversarial_trace(raw_outbound: bool = True):
    """(topology, events, labels): a mixed-protocol trace on a 200-pod / 1000-service graph plus eight hub pods with rows of the
    lengths in HUB_DEGREES, edges of 4095 / 4096 / 4097 events and errors, equal durations, means below, at and just above 100 ns,
    around 414.2 us (sg_log1p_pos's sqrt(1/2) split) and from 50 to 100 us, a max of 1e12 ns, z beyond +-8, sources with sd <= 1 us,
    open-connection-only pairs and (raw_outbound) raw-IP outbound destinations.  About 45 k events."""
    topo = replay.make_topology(200, 1500, seed=0x9B0E, svcs=1000)
    base, labels = replay.make_events(topo, 20_000, seed=0x9B0F, mixed=True, with_raw_outbound=raw_outbound, with_reverse=True)
    if not raw_outbound:                                             # (non-HTTP requests to unknown IPs carry no label: raw-IP nodes too)
        known = np.concatenate([topo.pod_ips, topo.svc_ips])
        base = base[(np.isin(base["saddr"], known) & np.isin(base["daddr"], known)) | (base["host_label"] != 0)]
    P, H = topo.n_pods, len(HUB_DEGREES)
    hub_ips = (replay.POD_IP_BASE + P + np.arange(H)).astype(np.uint32)
    cand = np.concatenate([topo.svc_ips, topo.pod_ips])
    rng = np.random.default_rng(0x9B10)
    parts, dsts = [base], []
    special = {4: 4, 6: 13, 7: 1}                                    # hub -> its first rows, whose events are placed below
    for h, deg in enumerate(HUB_DEGREES):
        dst = cand[rng.permutation(len(cand))[:deg]]
        dsts.append(dst)
        dur = np.rint(np.exp(np.log(5e6) + (0.01 if h == 0 else 0.3) * rng.standard_normal(deg))).astype(np.uint64)
        if h == 0:
            dur[7] = 60                                              # far below a narrow row: z < -8
        if h == 1:
            dur[3] = 1_000_000_000_000                               # max of 1e12 ns, z > 8
        if h == 5:
            dur[:] = 777_000; dur[9] = 779_000                       # the row's sd is below 1 us: z is m_e - mu
        k = special.get(h, 0)
        parts.append(_ev(deg - k, hub_ips[h], dst[k:], dur[k:]))
    # hub 4: edges of 4095 / 4096 / 4097 / 4200 events with 4095 / 4096 / 4096 / 4097 errors
    for i, (n, ne) in enumerate(((4095, 4095), (4096, 4096), (4097, 4096), (4200, 4097))):
        e = _ev(n, hub_ips[4], dsts[4][i], 1_000_000 + 1000 * i + np.arange(n, dtype=np.uint64) % 997)
        e["status"][:ne] = 503
        parts.append(e)
    # hub 7 (one edge): equal durations, std 0
    parts.append(_ev(3, hub_ips[7], dsts[7][0], 2500))
    # hub 6: edge means below, at and above 100 ns, from 50 to 100 us (sg_log1p_pos's series below 1e-4 ms), around 414.2 us
    means = (50, 99, 100, 101, 50_000, 60_000, 80_000, 95_000, 99_900, 414_200, 414_213, 414_214, 414_230)
    for i, m in enumerate(means):
        d = np.array([m, m, m + 3, m - 3] if m > 200 else [m, m], dtype=np.uint64)
        parts.append(_ev(len(d), hub_ips[6], dsts[6][i], d))
    # open connections only: busy pairs, idle pairs and (raw_outbound) raw IPs never seen otherwise (alive-only nodes)
    al = np.zeros(600, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[rng.integers(0, P, len(al))]                  # (not the hubs: their row lengths are set above)
    pick = rng.random(len(al))
    far = 0x5DB8D800 + rng.integers(0, 30, len(al)) if raw_outbound else topo.pod_ips[rng.integers(0, P, len(al))]
    al["daddr"] = np.where(pick < 0.6, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))],
                           np.where(pick < 0.85, topo.pod_ips[rng.integers(0, P, len(al))], far)).astype(np.uint32)
    parts.append(al)
    ev = np.concatenate(parts)
    ext = replay.Topology(P + H, topo.n_svcs, np.concatenate([topo.pod_ips, hub_ips]), topo.svc_ips, topo.edge_src, topo.edge_dst, topo.seed)
    return ext, ev, labels
