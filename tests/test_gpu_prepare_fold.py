"""Warm closes without the kc_prepare launch (alaz_amd/csrc/sg_plan.hpp Plan::prepare_fold, sg_k2.h kc_prepare_rest): on an unsharded
engine that keeps warm-window state, a close that tries the warm path launches no kc_prepare — that kernel's work is one more
workgroup of the warm attempt's launch, every merge workgroup takes the warm / cold decision itself, the window reset leaves C_COLD
and C_DELTA_N zero, and pass B's partition order is one window older (two buffers by window parity).

Every window here is closed by such an engine and by its twin, the same development build with SG_NO_FOLD=1 (the separate launch, as
every other close still has it).  Each window must match three ways: the rows byte for byte against the twin, the rows against the
oracle, and sg_stats — which path the window took, its new edges, drops, time range and node count — against the twin.

The graph is the smallest that still has several partitions in use and a row longer than one wave: 64 pods, 32 services, one pod that
talks to every other node, ~600 edges, 4 000 events a window, one layer.  The key-budget case needs tables that can run full:
SG_HT=256 (256 partitions of 208 keys) under two disjoint sets of 32 000 edges, one request each."""
import ctypes
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.helpers import CLOCK, HostShim, compare_edge_dicts, engine_edge_dict

pytestmark = pytest.mark.gpu

LAYERS = 1
KNOBS = ("SG_NO_FOLD", "SG_HT")
STATS = ("windows", "windows_warm", "windows_delta", "windows_cold", "windows_plain", "last_window_new_edges", "last_window_events",
         "last_window_edges", "last_window_nodes", "last_window_tmin_ms", "last_window_tmax_ms", "events_in", "events_dropped_src",
         "events_dropped_cap", "events_misrouted", "alive_in", "alive_dropped")


def _engine(topo, max_edges, fold, knobs=None, **kw):
    from alaz_amd import engine
    for k in KNOBS: os.environ.pop(k, None)
    os.environ.update(knobs or {})
    if not fold: os.environ["SG_NO_FOLD"] = "1"
    try:
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 16, max_edges=max_edges, layers=LAYERS, max_labels=256, max_outbound_ips=512,
                                k1_variant=3, warm=True, dev_knobs=True, **kw)
    finally:
        for k in KNOBS: os.environ.pop(k, None)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(LAYERS))
    geo = g.geometry()
    assert geo["warm_windows"] == 1 and geo["k1_narrow"] == 1 and geo["prepare_fold"] == int(fold), geo
    return g


class Trio:
    """an engine whose warm closes fold kc_prepare, its twin that launches it, and the oracle, fed the same windows"""
    def __init__(self, topo, max_edges, knobs=None, **kw):
        from oracle import pyoracle
        self.fold = _engine(topo, max_edges, True, knobs, **kw)
        self.twin = _engine(topo, max_edges, False, knobs, **kw)
        self.shim, self.shim2 = HostShim(), HostShim()
        self.o = pyoracle.Oracle(*CLOCK)
        self.W = weights.make_weights(LAYERS)
        ops = topo.k8s_ops()
        self.shim.apply(self.fold, ops); self.shim2.apply(self.twin, ops); self.o.apply_ops(ops)
        self.paths = []

    def stats(self):
        a, b = self.fold.stats(), self.twin.stats()
        sa, sb = {f: int(getattr(a, f)) for f in STATS}, {f: int(getattr(b, f)) for f in STATS}
        assert sa == sb, {f: (sa[f], sb[f]) for f in STATS if sa[f] != sb[f]}
        return sa

    def window(self, ev, labels, batches=1):
        before = self.stats()
        rows = []
        for g in (self.fold, self.twin):
            if len(ev):
                for part in np.array_split(ev, batches):
                    while g.ingest(np.ascontiguousarray(part)) != 0:
                        pass
            g.set_label_count(len(labels))
            rows.append(g.flush_window().copy())
        st = self.stats()
        assert st["windows"] == before["windows"] + 1
        kinds = [k for k in ("warm", "cold", "plain") if st["windows_" + k] > before["windows_" + k]]
        assert len(kinds) == 1, (before, st)
        delta = st["windows_delta"] > before["windows_delta"]
        assert delta == (st["last_window_new_edges"] > 0) and (not delta or kinds == ["warm"])
        self.paths.append("delta" if delta else kinds[0])
        assert rows[0].tobytes() == rows[1].tobytes(), "the folded close's rows differ from its twin's"
        self.o.packed(ev, labels); self.o.window_close(self.W, LAYERS)
        compare_edge_dicts(engine_edge_dict(rows[0], self.shim, labels, self.fold.outbound_ips()), self.o.edge_dict())
        orow = self.o.edge_rows()
        assert np.array_equal(rows[0]["from_ref"], orow["from_ref"]) and np.array_equal(rows[0]["to_ref"], orow["to_ref"])
        assert st["last_window_events"] == self.o.window_events and st["last_window_edges"] == len(rows[0]) == len(self.o.edge_dict())
        assert st["last_window_nodes"] == self.o.n_nodes
        assert np.array_equal(self.fold.outbound_ips(), self.twin.outbound_ips())
        return rows[0]

    def close(self):
        self.fold.close(); self.twin.close()


def _one_event_per_pair(src_ips, dst_ips, t0=2_000_000_000, label=0):
    n = len(src_ips)
    ev = np.zeros(n, dtype=replay.EVENT_DTYPE)
    ev["saddr"] = src_ips; ev["daddr"] = dst_ips
    ev["status"] = np.where(np.arange(n) % 17 == 0, 503, 200); ev["protocol"] = replay.PROTO_HTTP
    ev["host_label"] = label
    ev["duration_ns"] = 1_000_000 + (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(9_000_000))
    ev["write_time_ns"] = np.uint64(t0) + np.arange(n, dtype=np.uint64) * np.uint64(500)
    return ev


_CASE = {}


def _small_case():
    """the small graph and its windows, made once"""
    if not _CASE:
        topo = replay.make_topology(64, 500, seed=611, svcs=32)
        labels = list(replay.EXTERNAL_HOSTS)
        base, _ = replay.make_events(topo, 3_800, seed=612, fixed_labels=True)
        base = base[base["host_label"] <= 8]                            # the first windows know eight Host labels
        hub_dst = np.concatenate([topo.pod_ips[1:], topo.svc_ips])      # pod 0 talks to every other node: a row of 95 edges, longer than one wave
        hub = _one_event_per_pair(np.full(len(hub_dst), topo.pod_ips[0], dtype=np.uint32), hub_dst)
        first = np.concatenate([base, hub])
        seen = np.unique(first[["saddr", "daddr", "host_label"]])
        more, _ = replay.make_events(topo, 4_000, seed=613, fixed_labels=True)
        more = more[more["host_label"] <= 8]
        new = more[~np.isin(more[["saddr", "daddr", "host_label"]], seen)]
        assert len(new) > 20                                            # (pairs of the graph the first draw did not reach)
        raw = first[:3_000].copy()
        raw["daddr"][::300] = replay.EXTERNAL_IP_BASE + 0x100 + np.arange(len(raw["daddr"][::300]), dtype=np.uint32) * 7
        raw["host_label"][::300] = 0                                    # ten requests to raw outbound IPs
        lab, _ = replay.make_events(topo, 4_000, seed=614, fixed_labels=True)
        assert (lab["host_label"] > 8).any()                            # Host labels 9 .. 64 appear
        _CASE.update(topo=topo, labels=labels, first=first, new=np.concatenate([first[::2], new]), raw=raw, lab=lab)
        assert 550 <= len(seen) <= 700 and 3_500 <= len(first) <= 4_100, (len(seen), len(first))
    return _CASE


def test_every_kind_of_window_equals_the_twin_and_the_oracle():
    c = _small_case()
    L8, L64 = c["labels"][:8], c["labels"]
    p = Trio(c["topo"], 2048, max_window_events=1 << 16)
    try:
        r1 = p.window(c["first"], L8)                                   # nothing kept: cold, decided by every workgroup up front
        assert len(np.unique(r1["from_ref"], return_counts=True)[1]) > 1 and np.unique(r1["from_ref"], return_counts=True)[1].max() >= 95
        r2 = p.window(c["first"], L8)                                   # plain warm
        assert r1.tobytes() == r2.tobytes()
        p.window(c["new"], L8)                                          # edges the kept set lacks: delta
        assert p.paths == ["cold", "warm", "delta"], p.paths
        p.window(c["raw"], L8)                                          # raw outbound IPs: cold up front (the window word k1_resolve sets) ...
        assert p.paths[-1] == "cold" and len(p.fold.outbound_ips()) == 10
        p.window(c["first"], L8)                                        # ... the state that window left is not whole: rebuilt once more ...
        p.window(c["first"], L8)                                        # ... then warm again
        assert p.paths[-2:] == ["cold", "warm"], p.paths
        r = p.window(c["first"][:0], L8)                                # a window with no batch
        assert len(r) == 0 and p.paths[-1] == "warm"
        r = p.window(c["first"], L8, batches=3)                         # a window fed in three batches
        assert r.tobytes() == r1.tobytes() and p.paths[-1] == "warm"
        p.window(c["lab"], L64)                                         # new Host labels: the label count grows, their edges are new
        assert p.paths[-1] == "delta" and p.stats()["last_window_nodes"] == c["topo"].n_nodes + 64
        p.window(c["lab"], L64)
        assert p.paths[-1] == "warm"
        for g in (p.fold, p.twin): g.set_warm(False)                     # the host does not try: kc_prepare runs, the window is rebuilt
        p.window(c["first"], L64)
        for g in (p.fold, p.twin): g.set_warm(True)
        p.window(c["first"], L64)                                       # folded again, on the state the rebuild captured
        assert p.paths[-2:] == ["cold", "warm"], p.paths
        p.window(c["new"], L64)                                         # (the raw-IP window's rebuild started the kept set afresh: these edges are new again)
        p.window(c["new"], L64)                                         # (the order buffers of both parities have been through folded and separate closes)
        assert p.paths[-2:] == ["delta", "warm"], p.paths
        assert p.stats()["events_dropped_cap"] == 0
    finally:
        p.close()


def test_a_partition_beyond_its_key_budget_gives_up_after_the_merge():
    """C_COLD = 2, stored by a merge workgroup of a launch whose every workgroup had decided "warm": set A fills the partitions to 60 %,
    set B (none of A) does not fit beside it; the cold merge repeats the window and nothing is dropped; B again is warm."""
    topo = replay.make_topology(600, 64_000, seed=621, svcs=300)
    perm = np.random.default_rng(7).permutation(len(topo.edge_src))
    A, B = perm[:32_000], perm[32_000:]
    evA = _one_event_per_pair(topo.pod_ips[topo.edge_src[A]], topo.node_ip(topo.edge_dst[A]))
    evB = _one_event_per_pair(topo.pod_ips[topo.edge_src[B]], topo.node_ip(topo.edge_dst[B]))
    p = Trio(topo, 1 << 16, knobs={"SG_HT": "256"}, max_window_events=1 << 16)
    try:
        geo = p.fold.geometry()
        assert (geo["partitions"], geo["table_slots"], geo["pass_b_split"]) == (256, 256, 1), geo
        assert len(A) + len(B) > 256 * (256 * 13 // 16) + 8_192                # the tables cannot hold A and B together
        labels = list(replay.EXTERNAL_HOSTS)
        p.window(evA, labels); p.window(evB, labels); p.window(evB, labels)
        assert p.paths == ["cold", "cold", "warm"], p.paths
        assert p.stats()["events_dropped_cap"] == 0
    finally:
        p.close()


def test_two_windows_in_flight_each_slot_has_its_own_parity():
    """windows_in_flight = 2: window_run closes a window on its slot's stream and moves on; each slot counts its own closes (the parity of
    its order buffers) and keeps its own window words.  Four windows enqueued two at a time, then two through the synchronous API."""
    import torch
    c = _small_case()
    L8 = c["labels"][:8]
    wins = [c["first"], c["new"], c["first"], c["first"]]
    fold, twin = (_engine(c["topo"], 2048, f, max_window_events=1 << 16, windows_in_flight=2) for f in (True, False))
    one = _engine(c["topo"], 2048, False, max_window_events=1 << 16)
    try:
        for g in (fold, twin, one):
            HostShim().apply(g, c["topo"].k8s_ops()); g.set_label_count(len(L8))
        want = []
        for w in wins:
            assert one.ingest(w) == 0
            want.append(one.flush_window().copy())
        hip = ctypes.CDLL(None); hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in wins]
        torch.cuda.synchronize()
        for g in (fold, twin):
            for rnd in range(2):
                ptrs = []
                for k in range(2):
                    i = rnd * 2 + k
                    g.ingest_device(dev[i].data_ptr(), len(wins[i]), 0)
                    g.window_run(0)
                    ptrs.append(g.rows_buffer())
                torch.cuda.synchronize()
                assert len(set(ptrs)) == 2
                for k in range(2):
                    i = rnd * 2 + k
                    buf = np.zeros(len(want[i]), dtype=replay.EDGE_OUT_DTYPE)
                    assert len(buf) and hip.hipMemcpy(buf.ctypes.data, ctypes.c_void_p(ptrs[k]), len(buf) * 64, 2) == 0
                    assert buf.tobytes() == want[i].tobytes(), (i, g is fold)
        # the synchronous API on the current slot (slot 0 again: it has kept `first`): new edges, then nothing new
        for ev in (c["new"], c["first"]):
            rows, st = [], []
            for g in (fold, twin):
                assert g.ingest(ev) == 0
                rows.append(g.flush_window().copy())
                s = g.stats(); st.append({f: int(getattr(s, f)) for f in STATS if f not in ("events_in",)})
            assert rows[0].tobytes() == rows[1].tobytes() and st[0] == st[1], (st[0], st[1])
        assert (st[0]["windows_cold"], st[0]["windows_warm"], st[0]["windows_delta"]) == (0, 2, 1)
    finally:
        fold.close(); twin.close(); one.close()
