"""tests/halo_ref.py against tests/np_backend.py::NumpyBackend.halo_requests, on the CPU, on the traces tests/test_gpu_halo.py runs.

The two state the halo request lists separately — halo_ref from the unsharded window's rows (here: the oracle's), NumpyBackend from
one shard's own edges after the outbound-IP gather and the statistics all-reduce — and must agree before either judges the GPU.  The
shards are driven one after the other: the gather and the two all-reduces are the only points at which they meet."""
import numpy as np
import pytest
import torch

from alaz_amd import replay, sharded, weights
from oracle import pyoracle
from tests import halo_ref
from tests.helpers import CLOCK
from tests.np_backend import NumpyBackend


def _oracle_rows(topo, ev, labels):
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(1), 1)
    rows = o.edge_rows()
    return rows["from_ref"].copy(), rows["to_ref"].copy(), np.array(o.outbound_ips(), dtype=np.uint32), o.n_known, o.n_nodes


def _numpy_requests(topo, ev, n_labels, world):
    """the request lists of every shard by NumpyBackend: [r][k] = list of dense ids"""
    pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}; svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
    shard = sharded.route_events(ev, world, pod, svc)
    bes = [NumpyBackend(pod_ip_to_id=pod, svc_ip_to_id=svc, kind=[1] * topo.n_pods + [2] * topo.n_svcs, n_labels=n_labels,
                        weights=weights.make_weights(1), layers=1, rank=r, world=world, ncap=topo.n_nodes + n_labels + 4096, max_obip=4096)
           for r in range(world)]
    for r, be in enumerate(bes):
        be.ingest(ev[shard == r])
    assert sum(be.misrouted for be in bes) == 0
    ob = torch.stack([be.ob_local() for be in bes])
    for be in bes:
        be.ob_all.copy_(ob); be.close_gathered()
    s = torch.stack([be.stats_sum for be in bes]).sum(dim=0); m = torch.stack([be.stats_max for be in bes]).max(dim=0).values
    out = []
    for be in bes:
        be.stats_sum.copy_(s); be.stats_max.copy_(m); be.features()
        q = be.halo_requests().numpy()
        out.append([[int(x) for x in q[k, 1:1 + int(q[k, 0])]] for k in range(world)])
    return out, bes[0].N


def _unique_edges(ev):
    """one event per distinct (source, destination, label, direction, open-connection) combination: the lists depend on the edge SET
    only, and NumpyBackend ingests event by event in Python"""
    key = np.stack([ev["saddr"].astype(np.int64), ev["daddr"].astype(np.int64), ev["host_label"].astype(np.int64),
                    (ev["flags"] & (replay.EV_REVERSE | replay.EV_ALIVE)).astype(np.int64)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    return ev[np.sort(first)]


_TRACES = []


def _traces():
    """(name, (topo, events, labels), the oracle's rows of it), made once"""
    if not _TRACES:
        _TRACES.extend((name, tr, _oracle_rows(*tr)) for name, tr in _make_traces())
    return _TRACES


def _make_traces():
    for name, (p, e, n, seed) in halo_ref.TOPO_CASES.items():
        yield name, halo_ref.topo_trace(p, e, n, seed)
    yield "small", halo_ref.small_trace()
    topo, wins, labels = halo_ref.shrink_windows()
    for i, w in enumerate(wins):
        yield f"shrink{i}", (topo, w, labels)
    yield "shrink_repeat", (topo, wins[0], labels)                  # the warm engines' third window: the first one's trace again
    yield "one", halo_ref.one_trace()
    topo, ev, labels = halo_ref.topo_trace(*halo_ref.TOPO_CASES["t120"])
    yield "empty", (topo, ev[:0], labels)
    yield "large_map", halo_ref.large_map_trace()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_halo_ref_equals_numpy_backend_on_the_gpu_tests_traces(world):
    for name, (topo, ev, labels), (fr, to, ob, nk, n_nodes) in _traces():
        ref = halo_ref.HaloRef(fr, to, ob, nk, len(labels), world)
        assert ref.N == n_nodes and nk == topo.n_nodes, name
        got, n_np = _numpy_requests(topo, _unique_edges(ev), len(labels), world)
        assert n_np == ref.N, name
        for r in range(world):
            want = ref.req(r)
            assert got[r] == want, (name, r)
            assert want[r] == [] and all(l == sorted(set(l)) for l in want), (name, r)
            # the three lists of a shard hang together: what it scores = what it computes + what it asks for, nothing twice
            halo = sorted(x for l in want for x in l)
            assert sorted(ref.act_l(r) + halo) == ref.act_p(r) and not set(ref.act_l(r)) & set(halo), (name, r)
        # the GPU tests' precondition, from the reference: lists that are empty prove nothing
        ps = ref.pair_sizes()
        off = ps[~np.eye(world, dtype=bool)]
        if name in halo_ref.TOPO_CASES:
            assert (off > 0).all() if world < 8 else int((off > 0).sum()) >= 48, (name, ps)
        elif name in ("one", "empty"):
            assert ref.N == (1 if name == "one" else 180 + 64) and ps.sum() == 0, name
        else:
            assert off.sum() > 0, name


def test_capacities_cut_the_reference_lists_as_the_kernels_do():
    """the two clamps by hand on a six-row window at world 2 (hash32(0..3) % 2 decides who owns what, so the expectation is taken
    from the owners, not written down)"""
    fr = np.array([0, 1, 2, 3, 0, 1], dtype=np.uint32); to = np.array([1, 2, 3, 0, 2, 3], dtype=np.uint32)
    ref = halo_ref.HaloRef(fr, to, np.zeros(0, np.uint32), 4, 0, 2)
    for r in range(2):
        full = ref.req(r)
        k = 1 - r
        assert full[r] == [] and full[k] == sorted({int(t) for f, t in zip(fr, to) if ref.owner[f] == r and ref.owner[t] == k})
        cnt, ids, ovf = ref.padded(r, 1)
        assert cnt[k] == min(1, len(full[k])) and ids[k] == full[k][:1] and ovf == max(0, len(full[k]) - 1)
        cnt, ids = ref.unpadded(r, 1)
        assert sum(cnt) == min(1, len(full[k])) and ids == (full[0] + full[1])[:1]
    # owner order of the unpadded clamp: three owners' lists of 2, 3, 2 ids into room for 4
    class Fixed(halo_ref.HaloRef):
        def __init__(self): self.world = 3
        def req(self, r): return [[1, 2], [5, 6, 7], [8, 9]]
    assert Fixed().unpadded(0, 4) == ([2, 2, 0], [1, 2, 5, 6]) and Fixed().unpadded(0, 7) == ([2, 3, 2], [1, 2, 5, 6, 7, 8, 9])
    assert Fixed().unpadded(0, 1) == ([1, 0, 0], [1]) and Fixed().padded(0, 2) == ([2, 2, 2], [[1, 2], [5, 6], [8, 9]], 1)
