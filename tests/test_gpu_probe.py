"""Probe blobs on the GPU (tests/probe_weights.py): every scoring channel — node features of source and destination, the neighbour
means of one and two hops, the eight edge features, the constant head — read out per edge and held to the readout bound against
the oracle and the float64 reference, on every K1 variant, both model depths, both dense paths and both K4 forms, a warm window, the
logical shards (halo rows) and sg_window_run_sharded.  Also: weight reloads between windows and during a close (a close is scored
with the blob loaded when it began)."""
import ctypes
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.gpu_scaffold import _hip
from tests.helpers import CLOCK, HostShim, compare_edge_dicts, engine_edge_dict
from tests import probe_weights as pw

pytestmark = pytest.mark.gpu

_TRACE = {}
_ORACLE = {}


def _trace(raw_outbound=True):
    if raw_outbound not in _TRACE:
        _TRACE[raw_outbound] = pw.adversarial_trace(raw_outbound)
    return _TRACE[raw_outbound]


def _oracle_rows(layers, p, raw_outbound=True):
    """(rows, phi reference per row, phi the oracle's score reads out) of probe p; cached per trace, depth and probe"""
    key = (raw_outbound, layers, p.name)
    if key not in _ORACLE:
        from oracle import pyoracle
        topo, ev, labels = _trace(raw_outbound)
        o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(p.w, layers)
        rows = o.edge_rows()
        if p.kind == "const":
            ref = None
        elif p.kind == "edge":
            ref = pw.edge_features_ref(rows)[:, p.col]
        else:
            ref = pw.oracle_phi(p, o, rows)
        _ORACLE[key] = (rows, ref, None if ref is None else pw.readout(p, rows["score"]))
        o.close()
    return _ORACLE[key]


def check_probe(rows, layers, p, raw_outbound=True, where=""):
    """the engine's rows under probe p against the oracle's: same rows in the same order; recovered phi within the readout bound
    of the oracle's, and within it plus 1 fp32 ulp of the float64 reference (neighbour means: the oracle's pinned-order sums, so
    the bound alone)"""
    want, ref, phi_o = _oracle_rows(layers, p, raw_outbound)
    tag = f"{where} L={layers} {p.name}"
    assert len(rows) == len(want), tag
    assert np.array_equal(rows["from_ref"], want["from_ref"]) and np.array_equal(rows["to_ref"], want["to_ref"]), tag
    if p.kind == "const":
        assert np.array_equal(rows["score"], want["score"]), tag
        if not p.w.any():
            assert np.all(rows["score"] == np.float32(0.5)), tag
        return
    got = pw.readout(p, rows["score"])
    d = np.abs(got - phi_o)
    i = int(np.argmax(d))
    assert d[i] <= p.bound(), f"{tag}: |phi_gpu - phi_oracle| = {d[i]:.3e} > {p.bound():.3e} on row {i}: {rows[i]}"
    tol = p.bound() + (0.0 if p.kind in ("mean", "mean2", "selfmean") else pw.ulp32(ref))
    e = np.abs(got - pw.expected(p, ref)) - tol
    i = int(np.argmax(e))
    assert e[i] <= 0, f"{tag}: |phi_gpu - reference| = {e[i] + np.broadcast_to(tol, e.shape)[i]:.3e} on row {i}: {rows[i]} (ref {ref[i]!r})"


def _engine(layers, variant=3, **kw):
    from alaz_amd import engine
    topo, ev, labels = _trace(kw.pop("raw_outbound", True))
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=16384, layers=layers, max_labels=128, max_outbound_ips=512,
                            k1_variant=variant, max_window_events=len(ev) + 1, **kw)
    g.set_clock(*CLOCK)
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def _window(g, ev):
    assert g.ingest(ev) == 0
    return g.flush_window().copy()


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("layers", [1, 2])
def test_every_probe_on_every_k1_variant(layers, variant):
    """one window per probe blob, the same events every time, the blob reloaded in between"""
    _, ev, _ = _trace()
    g = _engine(layers, variant)
    for p in pw.probes(layers):
        g.load_weights(p.w)
        check_probe(_window(g, ev), layers, p, where=f"variant {variant}")
    g.close()


@pytest.mark.parametrize("valu", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_mean_probes_on_both_dense_paths_and_both_k4_forms(valu, fused):
    """K4's neighbour means through the MFMA and the VALU dense tiles, as one fused launch and as gather + tiles (the development
    build's SG_DENSE_VALU / SG_K4_FUSED knobs), both depths"""
    _, ev, _ = _trace()
    os.environ["SG_DENSE_VALU"] = valu; os.environ["SG_K4_FUSED"] = fused
    try:
        for layers in (1, 2):
            g = _engine(layers, dev_knobs=True)
            for p in pw.mean_probes(layers):
                g.load_weights(p.w)
                check_probe(_window(g, ev), layers, p, where=f"valu={valu} fused={fused}")
            g.close()
    finally:
        os.environ.pop("SG_DENSE_VALU", None); os.environ.pop("SG_K4_FUSED", None)


def test_every_probe_on_warm_windows():
    """the warm path (the kept CSR, delta windows): the trace without raw outbound IPs, so that every window after the first may
    take it; every probe's window is a warm one"""
    _, ev, _ = _trace(False)
    g = _engine(2, raw_outbound=False, warm=True)
    g.load_weights(weights.make_weights(2))
    _window(g, ev)
    for p in pw.probes(2):
        w0 = g.stats().windows_warm
        g.load_weights(p.w)
        check_probe(_window(g, ev), 2, p, raw_outbound=False, where="warm")
        assert g.stats().windows_warm == w0 + 1, "the window did not take the warm path"
    g.close()


def test_mean_probes_through_the_logical_shards():
    """G = 2 and 4 shard engines on one device (the halo rows: K6 packs a neighbour's layer output on its owner and unpacks it on
    the shard that gathers it): the concatenated rows under every mean probe, L = 2"""
    import threading
    import torch
    from alaz_amd import engine, sharded
    topo, ev, labels = _trace()
    layers = 2
    want = _oracle_rows(layers, pw.mean_probes(layers)[0])[0]
    pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}; svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
    dev = torch.device("cuda", 0)
    for world in (2, 4):
        shard = sharded.route_events(ev, world, pod, svc)
        ncap = topo.n_nodes + 8 + 128 + 512
        engs, bes = [], []
        for r in range(world):
            g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=16384, layers=layers, max_labels=128, max_outbound_ips=512,
                                    rank=r, world=world, max_window_events=len(ev))
            g.set_clock(*CLOCK); HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
            engs.append(g)
            bes.append(sharded.HipBackend(g, ncap=ncap, layers=layers, world=world, rank=r, device=dev, max_obip=512, stream=torch.cuda.Stream(dev)))
        for p in pw.mean_probes(layers):
            shared = sharded.ThreadComm.Shared(world)
            outs = [None] * world
            for r, g in enumerate(engs):
                g.load_weights(p.w)
                assert g.ingest(ev[shard == r]) == 0

            def run(r):
                sharded.run_window(bes[r], sharded.ThreadComm(shared, r))
                outs[r] = engs[r].window_read().copy()
                engs[r].window_reset(bes[r].s)
            ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
            for t in ths: t.start()
            for t in ths: t.join(timeout=300)
            assert all(o is not None for o in outs)
            got = np.concatenate(outs)
            got = got[np.lexsort((got["to_ref"], got["from_ref"]))]
            assert np.array_equal(np.lexsort((want["to_ref"], want["from_ref"])), np.arange(len(want)))
            check_probe(got, layers, p, where=f"world {world}")
        assert sum(e.stats().events_dropped_cap + e.stats().events_misrouted + e.stats().halo_overflow for e in engs) == 0
        torch.cuda.synchronize()
        for g in engs: g.close()


@pytest.mark.parametrize("layers", [1, 2])
def test_every_probe_through_window_run_sharded_at_world_1(layers):
    """sg_window_run_sharded with the library's own communicator at world = 1 (the staged pipeline with its collectives)"""
    import torch
    from alaz_amd import engine
    _, ev, _ = _trace()
    comm = engine.RcclComm(0, 1, 0, lambda raw: raw)
    g = _engine(layers, rank=0, world=1)
    st = torch.cuda.Stream(torch.device("cuda", 0))
    d = torch.from_numpy(ev.view(np.uint8).reshape(-1).copy()).cuda()
    for p in pw.probes(layers):
        g.load_weights(p.w)
        g.ingest_device(d.data_ptr(), len(ev), st.cuda_stream)
        g.window_run_sharded(comm, st.cuda_stream)
        check_probe(g.window_read().copy(), layers, p, where="sharded world 1")
    st.synchronize()
    comm.close(); g.close()


# ------------------------------------------------------------------------------------------------
# weight reloads
# ------------------------------------------------------------------------------------------------
def _blobs(layers):
    return weights.make_weights(layers), (weights.make_weights(layers, 0x5EED_0404) * np.float32(4)).astype(np.float32)


def _oracle_dicts(topo, ev, labels, layers, blobs):
    from oracle import pyoracle
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    out = []
    for w in blobs:
        o.packed(ev, labels); o.window_close(w, layers)
        out.append((o.edge_dict(), o.edge_rows()))
    o.close()
    return out


def _device_rows(hip, ptr, n):
    buf = np.zeros(n, dtype=replay.EDGE_OUT_DTYPE)
    assert hip.hipMemcpy(buf.ctypes.data, ctypes.c_void_p(ptr), n * 64, 2) == 0
    return buf


def test_blobs_alternate_between_windows_on_every_close_path():
    """blobs A and B loaded in turn before each window, on flush_window, flush_window_view, flush_begin / flush_end,
    flush_window_top, sg_window_run with one and with two windows in flight (rows from sg_window_rows_buffer) and the staged
    sg_window_* calls: every window equals the oracle under its own blob"""
    import torch
    topo, ev, labels = _trace()
    layers = 2
    A, B = _blobs(layers)
    (dA, rA), (dB, rB) = _oracle_dicts(topo, ev, labels, layers, (A, B))
    want = {0: (dA, rA), 1: (dB, rB)}

    def ok(rows, shim, g, which, path):
        d = want[which][0]
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), d)

    for path in ("flush_window", "view", "begin_end", "top"):
        g = _engine(layers); shim = HostShim(); shim.apply(g, topo.k8s_ops())
        for i in range(4):
            g.load_weights((A, B)[i & 1])
            assert g.ingest(ev) == 0
            if path == "flush_window":
                rows = g.flush_window().copy()
            elif path == "view":
                rows = g.flush_window_view().copy()
            elif path == "begin_end":
                g.flush_begin(); rows = g.flush_end().copy()
            else:
                rows, idx, n = g.flush_window_top(0)
                assert n == len(rows) == len(rA)
            ok(rows, shim, g, i & 1, path)
        g.close()

    hip = _hip()
    s = torch.cuda.current_stream().cuda_stream
    t = torch.from_numpy(ev.view(np.uint8).reshape(-1).copy()).cuda()
    for inflight in (1, 2):
        g = _engine(layers, windows_in_flight=inflight)
        ptrs = []
        for i in range(2 * inflight):
            g.load_weights((A, B)[i & 1])
            g.ingest_device(t.data_ptr(), len(ev), s)
            g.window_run(s)
            ptrs.append(g.rows_buffer())
            if inflight == 1:
                torch.cuda.synchronize()
                got = _device_rows(hip, ptrs[-1], len(rA))
                assert np.array_equal(got["from_ref"], rA["from_ref"])
                assert np.max(np.abs(got["score"] - want[i & 1][1]["score"])) <= 1e-5, (inflight, i)
        torch.cuda.synchronize()
        if inflight == 2:
            for i in (2, 3):
                got = _device_rows(hip, ptrs[i], len(rA))
                assert np.array_equal(got["from_ref"], rA["from_ref"])
                assert np.max(np.abs(got["score"] - want[i & 1][1]["score"])) <= 1e-5, (inflight, i)
        g.close()

    g = _engine(layers)
    for i in range(4):
        g.load_weights((A, B)[i & 1])
        g.ingest_device(t.data_ptr(), len(ev), s)
        g.window_close(s); g.window_features(s)
        for l in range(layers):
            g.window_layer(l, s)
        g.window_score(s)
        got = g.window_read().copy()
        g.window_reset(s)
        assert np.array_equal(got["from_ref"], rA["from_ref"]) and np.array_equal(got["to_ref"], rA["to_ref"])
        assert np.max(np.abs(got["score"] - want[i & 1][1]["score"])) <= 1e-5, ("staged", i)
    g.close()


def test_a_blob_loaded_during_a_close_applies_from_the_next_close():
    """the contract of sg_load_weights: a close is scored with the blob that was loaded when it began.  Blob B is loaded between
    sg_flush_begin and sg_flush_end of a config-2-sized window scored under A, and between two sg_window_run calls with two windows
    in flight: the first window equals the oracle under A, the next one under B"""
    import torch
    topo, ev, labels, layers = replay.make_config(2)
    A, B = _blobs(layers)
    (dA, rA), (dB, rB) = _oracle_dicts(topo, ev, labels, layers, (A, B))
    from alaz_amd import engine
    for inflight in (1, 2):
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=1 << 17, layers=layers, max_labels=128, max_outbound_ips=512,
                                k1_variant=3, max_window_events=len(ev) + 1, windows_in_flight=inflight)
        g.set_clock(*CLOCK)
        shim = HostShim(); shim.apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
        if inflight == 1:
            for _ in range(2):
                g.load_weights(A)
                for i in range(0, len(ev), 1 << 18):
                    assert g.ingest(ev[i:i + (1 << 18)]) == 0
                g.flush_begin()
                g.load_weights(B)                                   # while K4 / K5 of the window are still queued
                a = g.flush_end().copy()
                compare_edge_dicts(engine_edge_dict(a, shim, labels, g.outbound_ips()), dA)
                for i in range(0, len(ev), 1 << 18):
                    assert g.ingest(ev[i:i + (1 << 18)]) == 0
                b = g.flush_window().copy()
                compare_edge_dicts(engine_edge_dict(b, shim, labels, g.outbound_ips()), dB)
        else:
            hip = _hip()
            s = torch.cuda.current_stream().cuda_stream
            t = torch.from_numpy(ev.view(np.uint8).reshape(-1).copy()).cuda()
            for _ in range(2):
                g.load_weights(A)
                g.ingest_device(t.data_ptr(), len(ev), s)
                g.window_run(s); pa = g.rows_buffer()
                g.load_weights(B)                                   # window 1 still in flight
                g.ingest_device(t.data_ptr(), len(ev), s)
                g.window_run(s); pb = g.rows_buffer()
                torch.cuda.synchronize()
                for p, r in ((pa, rA), (pb, rB)):
                    got = _device_rows(hip, p, len(r))
                    assert np.array_equal(got["from_ref"], r["from_ref"]) and np.array_equal(got["to_ref"], r["to_ref"])
                    d = np.abs(got["score"].astype(np.float64) - r["score"])
                    assert d.max() <= 1e-5, (inflight, float(d.max()), int(np.argmax(d)))
        g.close()
