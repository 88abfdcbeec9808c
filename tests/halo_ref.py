"""What K6 must produce for a sharded window, restated in numpy and Python ints from the UNSHARDED window's rows (TEST INFRASTRUCTURE).

The input is the row list of the whole trace (from_ref / to_ref of the unsharded engine's or the oracle's rows), the sorted raw outbound
IPs of that window and the two node counts; nothing of a sharded run.  From these:

  dense index   KNOWN v -> v, LABEL v -> nk + v, OBIP v -> nk + nl + v (v = rank in the sorted union of raw outbound IPs, which is
                what a row's ref carries) — ref_of_dense of sg_kernels.h backwards, NumpyBackend._dense
  owner         hash32(ref) % world for KNOWN / LABEL nodes, sharded.owner_of_obip(ip) for OBIP nodes
  shard r       the rows whose `from` it owns
  od[v]         rows over all shards whose `from` is v (the all-reduced out-degree)

  req[r][k]     ascending { to of shard r : od[to] > 0 and owner(to) = k != r }        the rows r asks k for
  act_l[r]      ascending { from of shard r } + { to of shard r : od[to] = 0 }         layer outputs computed on r
  act_p[r]      ascending { from of shard r } + { to of shard r }                      score projections needed on r

and the two ways a list is cut short: the padded lists' capacity `capp` per (shard, owner) pair, the unpadded call's `cap` over the
whole concatenation.  tests/np_backend.py::NumpyBackend.halo_requests states the request lists a second time, from a shard's own
state after the exchanges; tests/test_halo_ref.py holds the two to one another before either judges the GPU."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from alaz_amd import replay, sharded

REF_KNOWN, REF_LABEL, REF_OBIP = 0, 1, 2


class HaloRef:
    def __init__(self, from_ref, to_ref, ob_ips, nk: int, nl: int, world: int):
        self.nk, self.nl, self.world = int(nk), int(nl), int(world)
        self.ob = np.asarray(ob_ips, dtype=np.uint32)
        assert (np.diff(self.ob.astype(np.int64)) > 0).all(), "the outbound IPs are the sorted union"
        self.N = self.nk + self.nl + len(self.ob)
        self.frm, self.to = self._dense(from_ref), self._dense(to_ref)
        v = np.arange(self.N, dtype=np.int64)
        ref = np.where(v < self.nk, v, (REF_LABEL << 30) | (v - self.nk)).astype(np.uint32)
        own = (replay.hash32(ref) % np.uint32(world)).astype(np.int64)
        if len(self.ob):
            own[self.nk + self.nl:] = sharded.owner_of_obip(self.ob, world).astype(np.int64)
        self.owner = own
        self.od = np.bincount(self.frm, minlength=self.N)
        self.shard_of_row = self.owner[self.frm] if len(self.frm) else np.zeros(0, dtype=np.int64)

    def _dense(self, ref) -> np.ndarray:
        ref = np.asarray(ref, dtype=np.int64)
        t, v = ref >> 30, ref & 0x3FFFFFFF
        assert ((t >= 0) & (t <= 2)).all() and (v[t == REF_KNOWN] < self.nk).all() and (v[t == REF_LABEL] < self.nl).all() \
            and (v[t == REF_OBIP] < len(self.ob)).all(), "a row names a node outside the window's numbering"
        return np.where(t == REF_KNOWN, v, np.where(t == REF_LABEL, self.nk + v, self.nk + self.nl + v))

    # ---- the lists ----
    def req(self, r: int) -> List[List[int]]:
        """req(r)[k]: what shard r asks owner k for, ascending (k = r: empty)"""
        to = np.unique(self.to[self.shard_of_row == r])
        need = to[(self.od[to] > 0) & (self.owner[to] != r)]
        return [[int(x) for x in need[self.owner[need] == k]] for k in range(self.world)]

    def act_l(self, r: int) -> List[int]:
        m = self.shard_of_row == r
        to = self.to[m]
        return [int(x) for x in np.unique(np.concatenate([self.frm[m], to[self.od[to] == 0]]))]

    def act_p(self, r: int) -> List[int]:
        m = self.shard_of_row == r
        return [int(x) for x in np.unique(np.concatenate([self.frm[m], self.to[m]]))]

    def pair_sizes(self) -> np.ndarray:
        """[r][k] = len(req(r)[k])"""
        return np.array([[len(l) for l in self.req(r)] for r in range(self.world)], dtype=np.int64)

    # ---- the two capacities ----
    def padded(self, r: int, capp: int) -> Tuple[List[int], List[List[int]], int]:
        """(count words, id lists, overflow) of shard r's padded lists with `capp` ids per owner: the count word is min(len, capp),
        the ids the first capp of the ascending list, the overflow the ids that did not fit, summed over the owners"""
        full = self.req(r)
        return [min(len(l), capp) for l in full], [l[:capp] for l in full], sum(max(0, len(l) - capp) for l in full)

    def unpadded(self, r: int, cap: int) -> Tuple[List[int], List[int]]:
        """(counts, ids) of the unpadded call with room for `cap` ids in all: the owners' lists fill ids in owner order, so ids is the
        first `cap` of their concatenation and counts[k] what of owner k's list lies before `cap` (k6_halo_build's clamp)"""
        full = self.req(r)
        counts, run = [], 0
        for l in full:
            counts.append(len(l) if run + len(l) <= cap else max(0, cap - run))
            run += len(l)
        return counts, [x for l in full for x in l][:cap]


# ------------------------------------------------------------------------------------------------
# the traces the halo tests run (tests/test_halo_ref.py on the CPU, tests/test_gpu_halo.py on the GPU)
# ------------------------------------------------------------------------------------------------
RAW_BASE = replay.EXTERNAL_IP_BASE + 0x4000       # raw outbound IPs of these traces: no pod, no service, no Host header


def outbound(topo, ips, n_plain: int, n_rev: int, seed: int) -> np.ndarray:
    """n_plain requests of pods to the raw IPs `ips` and n_rev reversed ones (the raw IP becomes the edge's from-endpoint, so the
    OBIP node has out-edges, is owned by the hash of its IP and turns up in the request lists at the top of the index range)"""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n_plain + n_rev, dtype=replay.EVENT_DTYPE)
    ev["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(ev))]
    ips = np.asarray(ips, dtype=np.uint32)
    ev["daddr"] = ips[np.arange(len(ev)) % len(ips)]
    ev["protocol"] = replay.PROTO_HTTP; ev["status"] = 200
    ev["duration_ns"] = rng.integers(1_000, 50_000_000, len(ev))
    ev["write_time_ns"] = 2_000_000_000 + np.arange(len(ev), dtype=np.uint64) * 100
    ev["protocol"][n_plain:] = replay.PROTO_AMQP; ev["status"][n_plain:] = 1; ev["flags"][n_plain:] = replay.EV_REVERSE
    return ev


def topo_trace(pods: int, edges: int, n_events: int, seed: int):
    """a make_topology graph with a mixed trace over it: Host labels, raw outbound IPs, reversed events, open connections"""
    topo = replay.make_topology(pods, edges, seed)
    ev, labels = replay.make_events(topo, n_events, seed + 1, mixed=True, with_raw_outbound=True, with_reverse=True, fixed_labels=True)
    ob = outbound(topo, RAW_BASE + np.arange(40, dtype=np.uint32) * 3, 400, 400, seed + 2)
    al = np.zeros(300, dtype=replay.EVENT_DTYPE)
    rng = np.random.default_rng(seed + 3)
    al["flags"] = replay.EV_ALIVE; al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
    al["daddr"] = topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))]
    h = n_events // 2
    return topo, np.concatenate([ev[:h], ob, al, ev[h:]]), labels


#: name -> (pods, edges, events, seed): 180 / 1 050 / 3 000 known nodes
TOPO_CASES = {"t120": (120, 1500, 12_000, 911), "t700": (700, 4000, 30_000, 921), "t2000": (2000, 8000, 50_000, 931)}


def small_trace(n_ob: int = 2, seed: int = 941):
    """60 known nodes, no Host labels and exactly n_ob raw outbound IPs: the label count alone then places N (N = 60 + labels + n_ob)"""
    topo = replay.make_topology(40, 300, seed)
    ev, _ = replay.make_events(topo, 3000, seed + 1, with_reverse=True)
    ext = (ev["daddr"] >= replay.EXTERNAL_IP_BASE) & (ev["daddr"] < replay.EXTERNAL_IP_BASE + 0x100)
    ev = ev[~ext]
    ev["host_label"] = 0
    ob = outbound(topo, RAW_BASE + np.arange(n_ob, dtype=np.uint32), 60, 60, seed + 2)
    return topo, np.concatenate([ev[:1500], ob, ev[1500:]]), []


def one_trace():
    """one registered pod that talks to itself: N = 1, one row on the shard that owns the pod, none elsewhere"""
    topo = replay.Topology(1, 0, np.array([replay.POD_IP_BASE], np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.int64), np.zeros(1, np.int64), 0)
    ev = np.zeros(50, dtype=replay.EVENT_DTYPE)
    ev["saddr"] = ev["daddr"] = replay.POD_IP_BASE; ev["protocol"] = replay.PROTO_HTTP; ev["status"] = 200; ev["duration_ns"] = 1000
    ev["write_time_ns"] = 2_000_000_000 + np.arange(50)
    return topo, ev, []


def shrink_windows(seed: int = 951):
    """three windows over one 180-node map whose N goes ~3000 -> ~500 -> ~3000.  An engine's label count never shrinks (kc_prepare
    keeps the largest it has seen), so the windows differ in their raw outbound IPs: 2 700, 250 and 2 650 of them, the third window's
    drawn from another range than the first's, with reversed events from a part of them."""
    topo = replay.make_topology(120, 1500, seed)
    labels = list(replay.EXTERNAL_HOSTS)
    wins = []
    for i, (n_ob, base) in enumerate(((2700, 0), (250, 1000), (2650, 5000))):
        ev, _ = replay.make_events(topo, 8000, seed + 10 + i, mixed=True, with_reverse=True, fixed_labels=True)
        ips = RAW_BASE + base + np.arange(n_ob, dtype=np.uint32)
        ob = outbound(topo, ips, n_ob + 300, n_ob // 2, seed + 20 + i)
        wins.append(np.concatenate([ev[:4000], ob, ev[4000:]]))
    return topo, wins, labels


def large_map_trace(seed: int = 961):
    """a map of 49 200 registered nodes (32 800 pods, 16 400 services) and a few thousand events over 4 000 of its edges: N > 49 152
    (K6_FLAGS_LDS), the one shape at which the one-workgroup builder takes its general form"""
    P, S, E = 32_800, 16_400, 4_000
    rng = np.random.default_rng(seed)
    src = rng.integers(0, P, E); dst = rng.integers(0, P + S, E)
    dst = np.where(dst == src, (dst + 1) % (P + S), dst)
    key = np.unique(src.astype(np.int64) << 32 | dst.astype(np.int64))
    topo = replay.Topology(P, S, (replay.POD_IP_BASE + np.arange(P, dtype=np.uint64)).astype(np.uint32),
                           (replay.SVC_IP_BASE + np.arange(S, dtype=np.uint64)).astype(np.uint32), key >> 32, key & 0xFFFFFFFF, seed)
    ev, labels = replay.make_events(topo, 6000, seed + 1, with_reverse=True, fixed_labels=True)
    ob = outbound(topo, RAW_BASE + np.arange(30, dtype=np.uint32), 200, 200, seed + 2)
    return topo, np.concatenate([ev[:3000], ob, ev[3000:]]), labels
