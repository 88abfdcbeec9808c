"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same traces.
Edge identities and integer accumulators bit-exact; fp32 scores within 1e-5 (north_star)."""
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.helpers import CLOCK, HostShim, compare_edge_dicts, engine_edge_dict

pytestmark = pytest.mark.gpu


def _engine(topo_nodes, max_edges, layers, **kw):
    from alaz_amd import engine
    # variant 0 here = the 8-byte-record path by name (3) with the warm-window state kept: sg_create's own rule would give engines of
    # these sizes the 16-byte kernels (variant 2 in the parametrised tests) and no kept state (test_k1_path_follows_the_window_size)
    if kw.get("k1_variant", 0) == 0:
        kw["k1_variant"] = 3
        kw.setdefault("warm", True)
    g = engine.ServiceGraph(max_known_nodes=topo_nodes, max_edges=max_edges, layers=layers,
                            max_labels=kw.pop("max_labels", 256), max_outbound_ips=kw.pop("max_outbound_ips", 512), **kw)
    g.set_clock(*CLOCK)
    g.load_weights(weights.make_weights(layers))
    return g


def _oracle(topo_ops, layers):
    from oracle import pyoracle
    o = pyoracle.Oracle(*CLOCK)
    o.apply_ops(topo_ops)
    return o


def _run_both(topo, batches, labels, layers, *, max_edges=None, chunk=1 << 18, variant=0):
    ops = topo.k8s_ops()
    g = _engine(topo.n_nodes + 8, max_edges or 4 * len(topo.edge_src) + 1024, layers, k1_variant=variant,
                max_window_events=max(len(b) for b in batches) + 1)
    shim = HostShim(); shim.apply(g, ops)
    o = _oracle(ops, layers)
    W = weights.make_weights(layers)
    worst = 0.0
    for ev in batches:
        for i in range(0, len(ev), chunk):              # ragged host batches through the staging ring
            rc = g.ingest(ev[i:i + chunk])
            while rc != 0:                               # SG_EAGAIN: ring full -> the test retries, production drops
                rc = g.ingest(ev[i:i + chunk])
        g.set_label_count(len(labels))
        rows = g.flush_window()
        o.packed(ev, labels)
        o.window_close(W, layers)
        got = engine_edge_dict(rows, shim, labels, g.outbound_ips())
        worst = max(worst, compare_edge_dicts(got, o.edge_dict()))
        st = g.stats()
        assert st.last_window_events == o.window_events
        assert st.last_window_edges == len(rows) == len(o.edge_dict())
        assert st.last_window_nodes == o.n_nodes
        if o.window_events:
            assert (st.last_window_tmin_ms, st.last_window_tmax_ms) == (o.window_tmin, o.window_tmax)
        assert np.array_equal(g.outbound_ips(), o.outbound_ips())
        # canonical order of the emitted rows == the oracle's row order
        assert np.array_equal(rows["from_ref"], o.edge_rows()["from_ref"]) and np.array_equal(rows["to_ref"], o.edge_rows()["to_ref"])
    return g, o, worst


def test_config1_full_reference_path():
    """BASELINE config 1: the oracle consumes the full 1096-byte wire records (payload parse, string
    tables — the reference's own path); the engine consumes the packed events."""
    from oracle import pyoracle
    topo, ev, labels, L = replay.make_config(1)
    g = _engine(topo.n_nodes + 8, 4096, L)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    assert g.ingest(ev) == 0
    g.set_label_count(len(labels))
    rows = g.flush_window()
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    o.l7_wire(replay.to_wire(ev, labels))
    assert o.labels == labels
    o.window_close(weights.make_weights(L), L)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    st = g.stats()
    assert st.events_dropped_src == o.dropped_src > 0 and st.events_in == len(ev)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("layers", [1, 2])
def test_edge_cases_mixed_trace(layers, variant):
    """raw-IP outbound, Host-header outbound, unknown sources, AMQP/Redis reversal, TLS, Kafka and
    Postgres status semantics, two windows, ragged batches."""
    topo = replay.make_topology(150, 1500, seed=31)
    ev1, labels = replay.make_events(topo, 60_000, seed=32, mixed=True, with_raw_outbound=True, with_reverse=True)
    ev2, labels2 = replay.make_events(topo, 45_001, seed=33, mixed=True, with_raw_outbound=True, with_reverse=True, stream_base=300)
    # second window reuses the first window's label table prefix (labels are cumulative)
    lab_all = list(labels)
    remap = np.zeros(len(labels2) + 1, dtype=np.uint32)
    for i, s in enumerate(labels2):
        if s not in lab_all:
            lab_all.append(s)
        remap[i + 1] = lab_all.index(s) + 1
    ev2 = ev2.copy(); ev2["host_label"] = remap[ev2["host_label"]]
    # oracle interns labels in first-use order: feed it the same cumulative table
    _run_both(topo, [ev1, ev2], lab_all, layers, chunk=7777, variant=variant)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_empty_and_tiny_windows(variant):
    topo = replay.make_topology(20, 40, seed=5)
    ev, labels = replay.make_events(topo, 3, seed=6)
    g, o, _ = _run_both(topo, [ev[:0], ev[:1], ev, ev[:0]], labels, 1, variant=variant)
    assert g.stats().windows == 4


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_table_updates_between_windows(variant):
    """ADD / UPDATE / DELETE between windows (persist.go:55-71,114-130), incl. an IP that is both a
    pod and a service (service wins, data.go:840-849) and a deleted source (events dropped)."""
    from alaz_amd import engine
    from oracle import pyoracle
    topo = replay.make_topology(30, 120, seed=9)
    ev, labels = replay.make_events(topo, 20_000, seed=10)
    ops0 = topo.k8s_ops()
    g = _engine(topo.n_nodes + 16, 4096, 1, k1_variant=variant)
    shim = HostShim(); shim.apply(g, ops0)
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(ops0)
    W = weights.make_weights(1)

    def window(e):
        assert g.ingest(e) == 0
        g.set_label_count(len(labels))
        rows = g.flush_window()
        o.packed(e, labels); o.window_close(W, 1)
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
        assert g.stats().last_window_events == o.window_events
    window(ev[:8000])
    pod0_ip = replay.ip_str(int(topo.pod_ips[0])); pod1_ip = replay.ip_str(int(topo.pod_ips[1]))
    ops1 = [("pod", "DELETE", topo.pod_uid(0), pod0_ip),                       # its events are dropped now
            ("svc", "ADD", "svc-shadowing-pod1", pod1_ip),                      # same IP as pod 1: service wins as destination
            ("pod", "UPDATE", topo.pod_uid(2), "10.9.9.9"),                     # pod 2 gets a second IP
            ("pod", "ADD", "pod-without-ip", "")]                               # skipped
    shim.apply(g, ops1); o.apply_ops(ops1)
    e2 = ev[8000:].copy()
    e2["saddr"][:50] = engine.ip_u32("10.9.9.9")
    window(e2)
    assert g.stats().events_dropped_src == o.dropped_src


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_config2_full_size_bit_exact_and_deterministic(variant):
    """BASELINE config 2 (1k pods / 50k edges / 1M events, L=1) against the oracle, run twice: the
    second run must reproduce the first bit for bit (integer atomics + canonical CSR order)."""
    topo, ev, labels, L = replay.make_config(2)
    g, o, worst = _run_both(topo, [ev], labels, L, max_edges=1 << 16, variant=variant)
    rows_a = None
    for _ in range(2):
        for i in range(0, len(ev), 1 << 18):
            assert g.ingest(ev[i:i + (1 << 18)]) == 0
        rows = g.flush_window()
        if rows_a is None:
            rows_a = rows.copy()
    assert rows.tobytes() == rows_a.tobytes()
    assert worst <= 1e-5
    # size-independent properties at full size
    acc = np.isin(ev["saddr"], topo.pod_ips)
    assert int(rows["count"].sum()) == int(acc.sum())
    assert int(rows["sum_ns"].sum()) == int(ev["duration_ns"][acc].astype(np.uint64).sum())
    assert int(rows["max_ns"].max()) == int(ev["duration_ns"][acc].max())
    assert int(rows["err_count"].sum()) == int((ev["status"][acc] >= 500).sum())


def test_mfma_dense_equals_valu_dense_bitwise():
    """K4/K5 dense blocks: v_mfma_f32_16x16x4_f32 chain vs a VALU fmaf chain, same k order."""
    topo = replay.make_topology(200, 3000, seed=41)
    ev, labels = replay.make_events(topo, 100_000, seed=42)
    out = []
    for valu in ("0", "1"):
        os.environ["SG_DENSE_VALU"] = valu
        try:
            g = _engine(topo.n_nodes + 8, 8192, 2)
            HostShim().apply(g, topo.k8s_ops())
            assert g.ingest(ev) == 0
            g.set_label_count(len(labels))
            out.append(g.flush_window().copy())
            g.close()
        finally:
            os.environ.pop("SG_DENSE_VALU", None)
    assert out[0].tobytes() == out[1].tobytes()


def test_k4_gather_launch_equals_the_fused_layer_bitwise():
    """K4 as two launches (k4_gather at high occupancy + dense tiles) vs the fused kernel (what small graphs still run):
    same block sums in the same order, so every row must be bit-identical — on a graph with rows shorter than one
    64-neighbour batch, of several batches and of more than one 512-neighbour block (the multi-block path of both)."""
    topo = replay.make_topology(600, 60_000, seed=43)           # Pareto out-degrees clipped at N/4 = 225 ...
    ev, labels = replay.make_events(topo, 400_000, seed=44)
    ev = ev.copy()
    hub = topo.pod_ips[0]                                        # ... so one source is made to talk to every service and pod
    dst = np.concatenate([topo.svc_ips, topo.pod_ips[1:]])
    ev["saddr"][:len(dst)] = hub; ev["daddr"][:len(dst)] = dst; ev["host_label"][:len(dst)] = 0; ev["flags"][:len(dst)] = 0
    out = []
    for fused in ("1", "0"):
        os.environ["SG_K4_FUSED"] = fused
        try:
            g = _engine(topo.n_nodes + 8, 1 << 17, 2, max_window_events=len(ev))
            HostShim().apply(g, topo.k8s_ops())
            for i in range(0, len(ev), 1 << 17):
                assert g.ingest(ev[i:i + (1 << 17)]) == 0
            g.set_label_count(len(labels))
            out.append(g.flush_window().copy())
            g.close()
        finally:
            os.environ.pop("SG_K4_FUSED", None)
    from collections import Counter
    deg = Counter(out[0]["from_ref"].tolist())
    assert max(deg.values()) > 512 and min(deg.values()) < 64, (max(deg.values()), min(deg.values()))
    assert out[0].tobytes() == out[1].tobytes()


def test_in_statistics_slice_counts_give_identical_rows():
    """The in-statistics are folded per (node range, edge slice) and the node features sum the slices' partials themselves (round 6: k3_in_reduce
    left the one-call pipelines; 48 slices where they are one round of the chip).  Integer sums and a maximum are order-free, so the rows must
    not depend on the slice count — 8 (the small-graph default), 33 and 47 (the sums' tail loop: not a multiple of four), 48."""
    topo = replay.make_topology(600, 60_000, seed=43)
    ev, labels = replay.make_events(topo, 400_000, seed=44)
    out = []
    for slices in (None, "33", "47", "48"):
        if slices: os.environ["SG_K3_SLICES"] = slices
        try:
            g = _engine(topo.n_nodes + 8, 1 << 17, 2, max_window_events=len(ev))
            HostShim().apply(g, topo.k8s_ops())
            for i in range(0, len(ev), 1 << 17):
                assert g.ingest(ev[i:i + (1 << 17)]) == 0
            g.set_label_count(len(labels))
            out.append(g.flush_window().copy())
            g.close()
        finally:
            os.environ.pop("SG_K3_SLICES", None)
    assert len(out[0]) > 30_000
    for o in out[1:]:
        assert out[0].tobytes() == o.tobytes()


def test_row_sort_by_blocks_equals_the_one_workgroup_row_sort_and_the_oracle():
    """Rows of more than 1024 edges are sorted a 512-edge block per workgroup (k2_row_block: every block ranks against the whole
    row's node bitmap, the row's out-statistics are summed with atomics and the last block derives row_mu / row_sd).  Against
    the single-workgroup row sort (SG_ABLATE bit 0x800) every row must be bit-identical, and against the oracle exact /
    within tolerance — on rows of 3599, 2100, 1025 and 1024 edges next to short ones, with error and duration tails."""
    topo = replay.make_topology(2400, 30_000, seed=71)
    ev, labels = replay.make_events(topo, 300_000, seed=72)
    ev = ev.copy()
    everyone = np.concatenate([topo.svc_ips, topo.pod_ips])
    at = 0
    for hub, n in ((5, 3599), (6, 2100), (7, 1025), (8, 1024)):
        dst = everyone[everyone != topo.pod_ips[hub]][:n]
        ev["saddr"][at:at + n] = topo.pod_ips[hub]; ev["daddr"][at:at + n] = dst; ev["host_label"][at:at + n] = 0; ev["flags"][at:at + n] = 0
        at += n
    out = []
    for ablate in ("0x800", None):
        if ablate: os.environ["SG_ABLATE"] = ablate
        try:
            g = _engine(topo.n_nodes + 8, 1 << 16, 2, max_window_events=len(ev))
            shim = HostShim(); shim.apply(g, topo.k8s_ops())
            for i in range(0, len(ev), 1 << 17):
                assert g.ingest(ev[i:i + (1 << 17)]) == 0
            g.set_label_count(len(labels))
            out.append(g.flush_window().copy())
            obips = g.outbound_ips()
            g.close()
        finally:
            os.environ.pop("SG_ABLATE", None)
    from collections import Counter
    deg = Counter(out[1]["from_ref"].tolist())
    top = sorted(deg.values())[-4:]
    assert top[-1] >= 3599 and top[-2] >= 2100 and top[0] >= 1024 and min(deg.values()) < 64, top
    assert out[0].tobytes() == out[1].tobytes()
    o = _oracle(topo.k8s_ops(), 2); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(out[1], shim, labels, obips), o.edge_dict())


def test_row_degrees_by_lds_histograms_equal_the_degree_atomics_and_the_oracle():
    """k2_deg_hist + k2_rowptr<64, DH> (row degrees and in-row ranks from LDS histograms, the default above 2^19 edges of capacity) forced
    on a small graph with SG_DH_G = 16 / 64 / 128 against the path with pass B's returning degree atomics (SG_DH_G=0, the default at this
    size): bit-identical rows — hub rows, rows of one edge, sources without any — and exact against the oracle.  (Config 3 at full size
    runs the histogram path by default; this keeps it covered where a failure is cheap to read.)"""
    topo = replay.make_topology(1800, 40_000, seed=81)
    ev, labels = replay.make_events(topo, 400_000, seed=82)
    ev = ev.copy()
    everyone = np.concatenate([topo.svc_ips, topo.pod_ips])
    n = 2500
    ev["saddr"][:n] = topo.pod_ips[3]; ev["daddr"][:n] = everyone[everyone != topo.pod_ips[3]][:n]; ev["host_label"][:n] = 0; ev["flags"][:n] = 0
    out = {}
    for dh in ("0", "16", "64", "128"):
        os.environ["SG_DH_G"] = dh
        try:
            g = _engine(topo.n_nodes + 8, 1 << 16, 2, max_window_events=len(ev))
            shim = HostShim(); shim.apply(g, topo.k8s_ops())
            for w in range(2):                                   # two windows: the histograms and the look-back epochs are re-armed
                for i in range(0, len(ev), 1 << 17):
                    assert g.ingest(ev[i:i + (1 << 17)]) == 0
                g.set_label_count(len(labels))
                out[(dh, w)] = g.flush_window().copy()
            obips = g.outbound_ips()
            g.close()
        finally:
            os.environ.pop("SG_DH_G", None)
    for dh in ("16", "64", "128"):
        for w in range(2):
            assert out[(dh, w)].tobytes() == out[("0", w)].tobytes(), (dh, w)
    assert out[("0", 0)].tobytes() == out[("0", 1)].tobytes()
    o = _oracle(topo.k8s_ops(), 2); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(out[("64", 1)], shim, labels, obips), o.edge_dict())


def test_pass_b_packed_add_equals_the_two_add_form_and_the_oracle():
    """Pass B adds a narrow record's count and duration in one 64-bit LDS operation (count in bits 48.., k1b_stream_merge<.., PACK>: the
    default wherever a workgroup merges fewer than 2^16 narrow records) or, with SG_K1B_PACK=0 and on larger geometries, as a 32-bit and a
    64-bit add.  Both forms must give bit-identical rows — a hot key the pass-A cache cannot hold (many records in one slot), second-long
    requests (sums far beyond 2^32), errors — and equal the oracle."""
    topo = replay.make_topology(1500, 30_000, seed=91)
    ev, labels = replay.make_events(topo, 500_000, seed=92)
    ev = ev.copy()
    ev["duration_ns"][::4] = 0xDC000000                                # 3.69 s: 2^16 of them would be 2^47.8 ns in one slot
    ev["status"][::9] = 503
    hot = slice(0, 120_000)                                             # one edge takes a quarter of the window
    ev["saddr"][hot] = topo.pod_ips[11]; ev["daddr"][hot] = topo.svc_ips[2]; ev["host_label"][hot] = 0; ev["flags"][hot] = 0
    out = {}
    for pack in ("0", None):
        if pack is not None: os.environ["SG_K1B_PACK"] = pack
        try:
            g = _engine(topo.n_nodes + 8, 1 << 16, 2, max_window_events=len(ev))
            shim = HostShim(); shim.apply(g, topo.k8s_ops())
            for i in range(0, len(ev), 1 << 17):
                assert g.ingest(ev[i:i + (1 << 17)]) == 0
            g.set_label_count(len(labels))
            out[pack] = g.flush_window().copy()
            obips = g.outbound_ips()
            g.close()
        finally:
            os.environ.pop("SG_K1B_PACK", None)
    assert out["0"].tobytes() == out[None].tobytes()
    assert int(out[None]["count"].max()) >= 100_000
    o = _oracle(topo.k8s_ops(), 2); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(out[None], shim, labels, obips), o.edge_dict())


def test_pass_b_second_long_requests_beside_ordinary_ones():
    """K1 pass B merges the 8-byte records with 32-bit LDS atomics on the low words of count / max and 64-bit ones on the sums, the
    wide records (durations beyond 2^32 ns) afterwards with 64-bit ones into the same slots.  A quarter of the requests take
    seconds (0xDC000000 ns: 1.36e13 us^2 each, sums far beyond 2^32), a few are beyond 2^32 ns, fed in 18 batches so that cache
    aggregates, single records and wide records meet in one table: every accumulator must equal the oracle's."""
    topo = replay.make_topology(200, 3000, seed=301)
    ev, labels = replay.make_events(topo, 120_000, seed=302)
    ev = ev.copy()
    rng = np.random.default_rng(303)
    hot = rng.choice(len(ev), 30_000, replace=False)
    ev["duration_ns"][hot] = rng.choice(np.array([0xDC000000, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 65_537_000], dtype=np.uint64), len(hot))
    ev["duration_ns"][rng.choice(len(ev), 300, replace=False)] = (1 << 33) + 12345
    g = _engine(topo.n_nodes + 8, 8192, 1, max_window_events=len(ev))
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    for i in range(0, len(ev), 7001):
        assert g.ingest(ev[i:i + 7001]) == 0
    g.set_label_count(len(labels))
    assert g.geometry()["k1_narrow"] == 1
    rows = g.flush_window()
    assert int(rows["sum_ns"].max()) > (1 << 36) and int(rows["sumsq_us"].max()) > (1 << 46)
    o = _oracle(topo.k8s_ops(), 1); o.packed(ev, labels); o.window_close(weights.make_weights(1), 1)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    g.close()


def test_flush_window_view_returns_the_same_rows_without_the_copy():
    """sg_flush_window_view: the rows of the window in the engine's page-locked buffer must be the rows sg_flush_window
    copies out — for a window, an empty window, and a larger one after it (the buffer grows); many feeder threads at once
    (any free staging slot is used, not only the next one in ring order)."""
    import threading
    topo = replay.make_topology(300, 9000, seed=61)
    ev, labels = replay.make_events(topo, 600_000, seed=62, mixed=True, with_raw_outbound=True)
    a = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=400_000, max_batch=1 << 14)
    b = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=400_000, max_batch=1 << 14)
    for g in (a, b):
        HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))

    def feed(g, e, threads):
        parts = np.array_split(np.arange(0, len(e), 1 << 14), threads) if len(e) else []
        def run(idx):
            for i in idx:
                while g.ingest(e[i:i + (1 << 14)]) != 0:
                    pass
        ths = [threading.Thread(target=run, args=(p,)) for p in parts]
        for t in ths: t.start()
        for t in ths: t.join()
    for lo, hi in ((0, 50_000), (50_000, 50_000), (50_000, 450_000)):
        feed(a, ev[lo:hi], 6); feed(b, ev[lo:hi], 1)
        v = a.flush_window_view(); c = b.flush_window()
        assert len(v) == len(c) and v.tobytes() == c.tobytes()
        assert not v.flags.writeable
    assert a.stats().events_dropped_cap == 0


def test_flush_begin_end_overlaps_the_next_windows_feed_without_mixing_windows():
    """sg_flush_begin marks the window boundary and returns with the pipeline enqueued; sg_flush_end_view fetches the rows
    without the engine lock while feeder threads already fill the next window.  Three windows fed that way (the fetch of
    window i running beside the feed of window i + 1, six feeder threads) must be byte for byte the rows of an engine that
    closes one window at a time — no batch slips across a boundary, no row is fetched late; also: the copy-out form
    (sg_flush_end), begin twice = SG_ESTATE, end without begin = SG_ESTATE, and sg_flush_window still works afterwards."""
    import threading
    from alaz_amd import engine
    topo = replay.make_topology(400, 20_000, seed=91)
    ev, labels = replay.make_events(topo, 900_000, seed=92, mixed=True, with_raw_outbound=True)
    a = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=400_000, max_batch=1 << 14)
    b = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=400_000, max_batch=1 << 14)
    for g in (a, b):
        HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    with pytest.raises(engine.ServiceGraphError) as ei:
        a.flush_end_view()
    assert ei.value.rc == engine.SG_ESTATE

    def feed(g, e, threads):
        parts = np.array_split(np.arange(0, len(e), 1 << 14), threads)
        def run(idx):
            for i in idx:
                while g.ingest(e[i:i + (1 << 14)]) != 0:
                    pass
        ths = [threading.Thread(target=run, args=(p,)) for p in parts]
        for t in ths: t.start()
        for t in ths: t.join()
    wins = [ev[0:300_000], ev[300_000:650_000], ev[650_000:900_000]]
    want = []
    for w in wins:
        feed(b, w, 1); want.append(b.flush_window().copy())
    got = []
    fetch = None
    def fetch_rows(): got.append(a.flush_end_view().copy())
    for w in wins:
        feed(a, w, 6)
        if fetch: fetch.join()
        a.flush_begin()
        with pytest.raises(engine.ServiceGraphError) as ei:
            a.flush_begin()
        assert ei.value.rc == engine.SG_ESTATE
        fetch = threading.Thread(target=fetch_rows); fetch.start()
    fetch.join()
    assert len(got) == 3
    for x, y in zip(got, want):
        assert len(x) == len(y) > 10_000 and x.tobytes() == y.tobytes()
    assert a.stats().windows == 3 and a.stats().events_dropped_cap == 0
    # the copying end, then the one-call close: same rows again
    feed(a, wins[0], 3); a.flush_begin(); r = a.flush_end()
    assert r.tobytes() == want[0].tobytes()
    feed(a, wins[1], 3)
    assert a.flush_window_view().tobytes() == want[1].tobytes()
    a.close(); b.close()


def test_device_resident_ingest_and_staged_pipeline():
    """sg_ingest_device on a torch-owned buffer + the staged window calls == sg_ingest + sg_flush_window."""
    import torch
    topo = replay.make_topology(80, 600, seed=51)
    ev, labels = replay.make_events(topo, 30_000, seed=52)
    g = _engine(topo.n_nodes + 8, 4096, 2)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    assert g.ingest(ev) == 0
    g.set_label_count(len(labels))
    a = g.flush_window().copy()
    t = torch.from_numpy(ev.view(np.uint8).reshape(-1)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    g.ingest_device(t.data_ptr(), len(ev), s)
    g.window_close(s); g.window_features(s)
    for l in range(2):
        g.window_layer(l, s)
    g.window_score(s)
    b = g.window_read().copy()
    g.window_reset(s)
    assert a.tobytes() == b.tobytes()
    # enqueue-only pipeline leaves the rows on the device
    g.ingest_device(t.data_ptr(), len(ev), s)
    g.window_run(s)
    torch.cuda.synchronize()
    rows = torch.empty(len(a) * 64, dtype=torch.uint8, device="cuda")
    import ctypes
    hip = ctypes.CDLL(None)          # the HIP runtime already loaded by torch / the engine
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(g.rows_buffer()), len(a) * 64, 3) == 0
    assert rows.cpu().numpy().tobytes() == a.tobytes()
    # staged calls with the reset folded into the score kernel (what the sharded driver's steady state uses):
    # same rows on the device, and the window is open and clean afterwards
    g.ingest_device(t.data_ptr(), len(ev), s)
    g.window_close(s); g.window_features(s)
    for l in range(2):
        g.window_layer(l, s)
    g.window_score_reset(s)
    torch.cuda.synchronize()
    assert hip.hipMemcpy(ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(g.rows_buffer()), len(a) * 64, 3) == 0
    assert rows.cpu().numpy().tobytes() == a.tobytes()
    assert g.ingest(ev[:1000]) == 0
    c = g.flush_window()
    assert int(c["count"].sum()) + int((np.isin(ev[:1000]["saddr"], topo.pod_ips) == False).sum()) == 1000


def test_capacity_overflow_is_counted_not_silent():
    topo = replay.make_topology(60, 800, seed=61)
    ev, labels = replay.make_events(topo, 30_000, seed=62)
    g = _engine(topo.n_nodes + 8, 256, 1, k1_variant=1)          # far fewer edge slots than edges
    HostShim().apply(g, topo.k8s_ops())
    assert g.ingest(ev) == 0
    rows = g.flush_window()
    st = g.stats()
    assert len(rows) == 256 and st.events_dropped_cap > 0
    # the next window starts clean
    assert g.ingest(ev[:10]) == 0
    assert len(g.flush_window()) <= 10


@pytest.mark.parametrize("pods,edges,events,cap", [(1000, 50_000, 600_000, 8192), (2000, 300_000, 1_500_000, 140_000)])
def test_edge_capacity_overflow_many_times_over_is_counted_and_stays_in_bounds(pods, edges, events, cap):
    """A window with several times more distinct edges than max_edges (variant 0: pass B finds them all, the CSR holds max_edges):
    k2_rowptr publishes row starts clamped to the capacity, so the rows behind it are empty for every later kernel.  (Unclamped,
    the SAGE gather walked the column array up to the number of edges FOUND — a GPU memory fault when bench.py's feeders put ten
    traces into one C2-sized window.)  Both K4 forms (fused below 2^17 edge slots, gather + dense above) and a hub row across
    the boundary; the engine must report max_edges rows, count the rest, keep every row a distinct edge with its own events,
    and start the next window clean (checked against the oracle)."""
    topo = replay.make_topology(pods, edges, seed=401)
    ev, labels = replay.make_events(topo, events, seed=402)
    ev = ev.copy()
    hub = topo.pod_ips[pods // 2]                                   # a row of N - 1 edges somewhere in the middle of the id space
    dst = np.concatenate([topo.svc_ips, topo.pod_ips[topo.pod_ips != hub]])
    ev["saddr"][:len(dst)] = hub; ev["daddr"][:len(dst)] = dst; ev["host_label"][:len(dst)] = 0; ev["flags"][:len(dst)] = 0
    g = _engine(topo.n_nodes + 8, cap, 2, max_window_events=len(ev), max_batch=1 << 18)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    for i in range(0, len(ev), 1 << 18):
        assert g.ingest(ev[i:i + (1 << 18)]) == 0
    g.set_label_count(len(labels))
    rows = g.flush_window()
    st = g.stats()
    assert len(rows) == cap and st.events_dropped_cap > 0 and st.last_window_edges == cap
    pairs = rows["from_ref"].astype(np.uint64) << np.uint64(32) | rows["to_ref"].astype(np.uint64)
    assert len(np.unique(pairs)) == cap                                                       # every row a distinct edge
    assert int(rows["count"].sum()) + int(st.events_dropped_cap) <= len(ev) and np.isfinite(rows["score"]).all()
    # the next window is an ordinary one
    small = ev[len(dst):len(dst) + 3000]
    assert g.ingest(small) == 0
    rows2 = g.flush_window()
    o = _oracle(topo.k8s_ops(), 2); o.packed(small, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(rows2, shim, labels, g.outbound_ips()), o.edge_dict())
    g.close()


def test_partitioned_k1_overflow_paths_are_exact_or_counted():
    """Variant 0 with deliberately tiny slab pieces (max_window_events far below the real load):
    records spill into the overflow list and the result must still be bit-exact; when even that
    list is exhausted the loss must show up in events_dropped_cap, never silently."""
    from oracle import pyoracle
    topo = replay.make_topology(100, 2000, seed=71)
    ev, labels = replay.make_events(topo, 200_000, seed=72)
    g = _engine(topo.n_nodes + 8, 8192, 1, k1_variant=0, max_window_events=20_000)   # pieces sized for 10x fewer events
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    assert g.ingest(ev) == 0
    g.set_label_count(len(labels))
    rows = g.flush_window()
    st = g.stats()
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(1), 1)
    if st.events_dropped_cap == 0:
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    else:
        assert int(rows["count"].sum()) + st.events_dropped_cap == o.window_events


def test_cpp_graphds_end_to_end_from_wire_records():
    """The product path end to end: 1096-byte l7_event records -> C++ GraphDS (L7 packer, id interning,
    batching) -> C ABI -> HIP kernels -> EdgeSink rows, against the oracle's full reference path on the
    same records (payload parse, string tables, setFromToV2), incl. SQL drops, Kafka fan-out, reversal."""
    from alaz_amd import engine, hostlib
    from oracle import pyoracle
    topo = replay.make_topology(60, 400, seed=11)
    ev, labels = replay.make_events(topo, 20_000, seed=12, mixed=True, with_raw_outbound=True, with_reverse=True)
    wire = bytearray(replay.to_wire(ev, labels))
    pg = np.flatnonzero(ev["protocol"] == replay.PROTO_POSTGRES)[:50]
    for j, i in enumerate(pg):
        off = int(i) * replay.L7_WIRE_SIZE
        if j % 2:
            wire[off + 36 + 5: off + 36 + 11] = b"xxxxxx"
        else:
            wire[off + 1060: off + 1064] = (3).to_bytes(4, "little")
    kafka = np.where(ev["protocol"] == replay.PROTO_KAFKA, 1 + (np.arange(len(ev)) % 3), 1).astype(np.uint32)
    wire = bytes(wire)
    W = weights.make_weights(2)
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.l7_wire(wire, kafka); o.window_close(W, 2)
    cfg = engine.make_config(max_known_nodes=topo.n_nodes + 8, max_edges=4096, layers=2, max_outbound_ips=256, max_window_events=1 << 16)
    g = hostlib.GraphDS(cfg, batch=1000)
    g.set_clock(*CLOCK); g.load_weights(W)
    g.apply_ops(topo.k8s_ops())
    assert g.ingest_wire(wire, kafka) == 0
    got = g.FlushWindow(123)
    compare_edge_dicts(got, o.edge_dict())
    assert g.dropped_parse == o.dropped_parse > 0 and g.labels == o.labels
    # f-2, second window: TCP connect records -> socket lines -> sweep -> alive connections beside the requests
    from tests.helpers import _tcp_wire
    rng = np.random.default_rng(5)
    ips = [replay.ip_str(int(x)) for x in topo.pod_ips[:20]] + [replay.ip_str(int(x)) for x in topo.svc_ips[:10]] + ["93.184.216.34", "172.16.5.5"]
    recs = []
    for k in range(400):
        recs.append((1 if rng.random() < 0.7 else 5, int(rng.integers(1, 9)), int(rng.integers(3, 20)), 1000 + 7 * k,
                     ips[int(rng.integers(0, 20))] if rng.random() < 0.9 else ips[-1], 40000 + k, ips[int(rng.integers(0, len(ips)))], 443))
    tw = _tcp_wire(recs)
    assert g.tcp_wire(tw) == o.tcp_wire(tw)
    assert g.ingest_wire(wire[: 5000 * replay.L7_WIRE_SIZE], kafka[:5000]) == 0
    o.l7_wire(wire[: 5000 * replay.L7_WIRE_SIZE], kafka[:5000])
    g.sweep(99); o.sweep(99)
    o.window_close(W, 2)
    got = g.FlushWindow(124)
    compare_edge_dicts(got, o.edge_dict())
    assert sum(v[8] for v in got.values()) == o.alive_count() > 0
    # f-4, third window: real HTTP/2 frames (HPACK) and Kafka payloads (record batches, compressed) decoded on the host
    from tests.h2_builder import _h2_trace
    from tests import kafka_builder as kb
    h2_wire, pids = _h2_trace(topo, 300, seed=8)
    rk = np.random.default_rng(9); krecs = []
    for i in range(300):
        batch = [kb.record(b"k%d" % j, b"v" * 12, offset_delta=j) for j in range(int(rk.integers(1, 6)))]
        codec = int(rk.integers(0, 5)); s_ip = int(topo.pod_ips[int(rk.integers(0, 30))]); d_ip = int(topo.svc_ips[int(rk.integers(0, 5))])
        if i % 2:
            krecs.append(kb.l7_record(2, kb.fetch_response([(b"orders", [(i % 4, kb.record_batch(batch, codec=codec))])]), 10_000_000 + i, s_ip, d_ip, api_version=11))
        else:
            krecs.append(kb.l7_record(1, kb.produce_request([(b"orders", [(i % 4, kb.record_batch(batch, codec=codec))])]), 10_000_000 + i, s_ip, d_ip, api_version=7))
    krecs.append(kb.l7_record(1, b"\x00\x00\x00\x09not kafka", 10_000_999, int(topo.pod_ips[0]), int(topo.svc_ips[0])))
    w3 = h2_wire + b"".join(krecs)
    o.set_kafka_decode(True); g.kafka_decode(True)
    for p in pids:
        o.h2().proc_exec(p); g.proc_exec(p)
    d0 = o.dropped_parse
    n3 = o.l7_wire(w3); assert g.ingest_wire(w3) == 0
    o.window_close(W, 2)
    got = g.FlushWindow(125)
    compare_edge_dicts(got, o.edge_dict())
    assert n3 > 900 and g.dropped_parse == o.dropped_parse == d0 + 1 and g.labels == o.labels and g.http2_stats()["pending"] == 0
    # f-3: the same rows as "/edges/" payloads (edges_payload.hpp)
    import json, struct
    f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
    docs = [json.loads(d) for d in g.edges_json("mon", "key", "node", "v", batch=100)]
    assert len(docs) == -(-len(got) // 100) and all(d["window_end"] == 125 for d in docs)
    from_json = {(e[0], e[1], e[2], e[3]): (e[4], e[5], e[6], e[7], e[8], f32(e[10]), f32(e[11]), f32(e[12]), e[9], e[13], e[14]) for d in docs for e in d["edges"]}
    assert from_json == got


@pytest.mark.parametrize("layers", [1, 2])
def test_logical_shards_on_one_device_equal_the_unsharded_engine(layers):
    """SURVEY.md §8e validation: G = 2 and G = 4 shard engines on ONE device (one thread per shard,
    the real HipBackend + exchange logic, collectives through ThreadComm) must reproduce the unsharded
    engine bit for bit: integer statistics are exact and halo rows are copied, never reduced."""
    import threading
    import torch
    from alaz_amd import engine, sharded
    topo = replay.make_topology(120, 1500, seed=91)
    ev, labels = replay.make_events(topo, 60_000, seed=92, mixed=True, with_raw_outbound=True, with_reverse=True, fixed_labels=True)
    # f-2: open connections too — on busy edges, on idle pairs, to raw outbound IPs; a stray REVERSE flag must not
    # change where they are routed (K1 never reverses an alive record)
    rng = np.random.default_rng(94)
    al = np.zeros(4000, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE; al["flags"][::5] |= replay.EV_REVERSE
    al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
    pick = rng.random(len(al))
    al["daddr"] = np.where(pick < 0.5, topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))],
                  np.where(pick < 0.8, topo.pod_ips[rng.integers(0, topo.n_pods, len(al))], 0x5DB8D800 + rng.integers(0, 30, len(al)))).astype(np.uint32)
    ev = np.concatenate([ev[:30_000], al[:2000], ev[30_000:], al[2000:]])
    W = weights.make_weights(layers)
    ref = _engine(topo.n_nodes + 8, 8192, layers, max_labels=128, max_outbound_ips=512)
    shim = HostShim(); shim.apply(ref, topo.k8s_ops())
    assert ref.ingest(ev) == 0
    ref.set_label_count(len(labels))
    want = ref.flush_window()
    for world in (2, 4):
        shard = ref.route(ev, world)
        pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}; svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
        assert np.array_equal(shard, sharded.route_events(ev, world, pod, svc))     # host twin == sg_route
        shared = sharded.ThreadComm.Shared(world)
        dev = torch.device("cuda", 0)
        ncap = topo.n_nodes + 8 + 128 + 512
        engs, bes, outs = [], [], [None] * world
        for r in range(world):
            g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=8192, layers=layers, max_labels=128, max_outbound_ips=512,
                                    rank=r, world=world, max_window_events=len(ev))
            g.set_clock(*CLOCK); g.load_weights(W); HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
            assert g.ingest(ev[shard == r]) == 0
            engs.append(g)
            bes.append(sharded.HipBackend(g, ncap=ncap, layers=layers, world=world, rank=r, device=dev, max_obip=512, stream=torch.cuda.Stream(dev)))

        def run(r):
            sharded.run_window(bes[r], sharded.ThreadComm(shared, r))
            outs[r] = engs[r].window_read().copy()
            engs[r].window_reset(bes[r].s)
        ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in ths: t.start()
        for t in ths: t.join(timeout=300)
        assert all(o is not None for o in outs)
        assert sum(e.stats().events_dropped_cap + e.stats().events_misrouted for e in engs) == 0
        got = np.concatenate(outs)
        key = lambda a: np.lexsort((a["to_ref"], a["from_ref"]))
        got = got[key(got)]; exp = want[key(want)]
        assert len(got) == len(exp) and min(len(o) for o in outs) > 0
        assert got.tobytes() == exp.tobytes()
        assert int(got["alive"].sum()) == len(al) and sum(e.stats().alive_in for e in engs) == len(al)
        for g in engs: g.close()


def test_outbound_ip_capacity_overflow_is_counted():
    """More distinct raw outbound IPs than max_outbound_ips: the unlisted ones are dropped and counted,
    the listed ones keep exact results (no aliasing of node ids)."""
    from oracle import pyoracle
    topo = replay.make_topology(40, 200, seed=81)
    ev, labels = replay.make_events(topo, 20_000, seed=82, with_raw_outbound=True)
    for variant in (0, 1, 2):
        g = _engine(topo.n_nodes + 8, 4096, 1, max_outbound_ips=16, k1_variant=variant)
        shim = HostShim(); shim.apply(g, topo.k8s_ops())
        assert g.ingest(ev) == 0
        g.set_label_count(len(labels))
        rows = g.flush_window()
        st = g.stats()
        o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(1), 1)
        assert len(g.outbound_ips()) == 16 and len(o.outbound_ips()) > 16 and st.events_dropped_cap > 0
        assert int(rows["count"].sum()) + st.events_dropped_cap == o.window_events
        want = o.edge_dict()
        got = engine_edge_dict(rows, shim, labels, g.outbound_ips())
        assert set(got) <= set(want) and all(got[k][:5] == want[k][:5] for k in got)


def _feed(g, ev, chunk=1 << 18):
    for i in range(0, len(ev), chunk):
        while g.ingest(ev[i:i + chunk]) != 0:
            pass


def _c3_engine_and_rows(n_events):
    topo = replay.make_topology(10_000, 1_000_000, replay.SEED_BASE + 3)
    ev, labels = replay.make_events(topo, n_events, replay.SEED_BASE + 3)
    g = _engine(topo.n_nodes, 1_250_000, 2, max_labels=128, max_outbound_ips=128, max_window_events=len(ev))
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    _feed(g, ev)
    g.set_label_count(len(labels))
    return topo, ev, labels, g, g.flush_window()


def test_config3_full_size_row_for_row_against_the_oracle():
    """BASELINE config 3 at FULL size — 10k pods / 5k services / 1M edges (power-law out-degree up to 3750), 10M events,
    2 SAGE layers, fed as 40 host batches — row for row against the oracle: every edge identity, every integer
    accumulator, err_ratio bit-exact; score within 1e-5, lat_z within 1e-5 relative (north_star).  Rows come out in
    the same canonical order, so the arrays are compared directly (~1.0 M rows)."""
    from oracle import pyoracle
    topo, ev, labels, g, rows = _c3_engine_and_rows(10_000_000)
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    want = o.edge_rows()
    st = g.stats()
    assert st.events_dropped_cap == 0 and st.last_window_events == o.window_events and len(rows) == len(want) > 1_000_000
    assert st.events_dropped_src == o.dropped_src and st.last_window_nodes == o.n_nodes
    for f in ("from_ref", "to_ref", "count", "err_count", "sum_ns", "max_ns", "sumsq_us", "err_ratio"):
        assert np.array_equal(rows[f], want[f]), f
    assert np.abs(rows["score"] - want["score"]).max() <= 1e-5
    assert (np.abs(rows["lat_z"] - want["lat_z"]) <= 1e-5 * np.maximum(1.0, np.abs(want["lat_z"]))).all()


def test_config3_full_size_invariants():
    """BASELINE config 3 at full size (10M events, 1M edges, L=2): size-independent properties — event
    conservation, checksums of the integer accumulators against numpy, canonical strictly increasing
    row order, scores inside (0, 1)."""
    topo, ev, labels, g, rows = _c3_engine_and_rows(10_000_000)
    st = g.stats()
    acc = np.isin(ev["saddr"], topo.pod_ips)
    assert st.events_dropped_cap == 0 and st.events_dropped_src == int((~acc).sum())
    assert int(rows["count"].astype(np.uint64).sum()) == int(acc.sum()) == st.last_window_events
    assert int(rows["sum_ns"].sum()) == int(ev["duration_ns"][acc].sum())
    us = ev["duration_ns"][acc] // np.uint64(1000)
    assert int(rows["sumsq_us"].sum()) == int((us * us).sum())
    assert int(rows["max_ns"].max()) == int(ev["duration_ns"][acc].max())
    assert int(rows["err_count"].sum()) == int((ev["status"][acc] >= 500).sum())
    NK, NL = topo.n_nodes, len(labels)

    def dense(ref):
        t, v = ref >> 30, (ref & 0x3FFFFFFF).astype(np.int64)
        return np.where(t == 0, v, np.where(t == 1, NK + v, NK + NL + v))
    key = dense(rows["from_ref"]) * (1 << 20) + dense(rows["to_ref"])
    assert (np.diff(key) > 0).all()
    assert ((rows["score"] > 0) & (rows["score"] < 1)).all() and np.isfinite(rows["lat_z"]).all()
    key_ev = np.unique((ev["saddr"][acc].astype(np.uint64) << np.uint64(32)) | ev["daddr"][acc].astype(np.uint64))
    assert len(rows) == len(key_ev)                 # HTTP-only trace: one edge per distinct (saddr, daddr) of accepted events


def _logical_shards(topo, ev, labels, layers, world, *, max_edges, max_labels=128, max_obip=128):
    """`world` shard engines on ONE device, one thread per shard, the real HipBackend + exchange logic with the
    collectives going through ThreadComm; returns the concatenated rows and the engines' summed drop counters."""
    import threading
    import torch
    from alaz_amd import engine, sharded
    W = weights.make_weights(layers)
    pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}; svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
    shard = sharded.route_events(ev, world, pod, svc)
    shared = sharded.ThreadComm.Shared(world)
    dev = torch.device("cuda", 0)
    ncap = topo.n_nodes + max_labels + max_obip
    engs, bes, outs = [], [], [None] * world
    for r in range(world):
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=max_edges, layers=layers, max_labels=max_labels, max_outbound_ips=max_obip,
                                rank=r, world=world, max_window_events=int((shard == r).sum()) + 1)
        g.set_clock(*CLOCK); g.load_weights(W); HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
        _feed(g, ev[shard == r])
        engs.append(g)
        bes.append(sharded.HipBackend(g, ncap=ncap, layers=layers, world=world, rank=r, device=dev, max_obip=max_obip, stream=torch.cuda.Stream(dev)))

    def run(r):
        sharded.run_window(bes[r], sharded.ThreadComm(shared, r))
        outs[r] = engs[r].window_read().copy()
        engs[r].window_reset(bes[r].s)
    ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ths: t.start()
    for t in ths: t.join(timeout=600)
    assert all(o is not None for o in outs)
    bad = sum(e.stats().events_dropped_cap + e.stats().events_misrouted + e.stats().halo_overflow for e in engs)
    for g in engs: g.close()
    return np.concatenate(outs), bad, [len(o) for o in outs]


def test_config4_eight_logical_shards_of_the_config3_graph_equal_one_engine():
    """BASELINE config 4 = config 3's graph hash-sharded by source pod over 8 GPUs.  Here: 8 logical shards on one
    device (SURVEY.md §8e validation), 4 M events, 2 layers — the concatenated rows must equal the unsharded
    engine's bit for bit (halo rows are copied, never reduced; integer statistics are exact), with the halo capacity
    the multi-GPU bench uses (sized from the node space / world) and no overflow."""
    topo, ev, labels, g, want = _c3_engine_and_rows(4_000_000)
    g.close()
    got, bad, per = _logical_shards(topo, ev, labels, 2, 8, max_edges=1_250_000 // 4)
    assert bad == 0 and min(per) > 50_000
    key = lambda a: np.lexsort((a["to_ref"], a["from_ref"]))
    got = got[key(got)]; exp = want[key(want)]
    assert len(got) == len(exp) > 800_000
    assert got.tobytes() == exp.tobytes()


def test_config5_mixed_protocol_window_on_the_global_table_path_against_the_oracle():
    """BASELINE config 5's graph at full size (100k pods / 50k services / 20M edges) with one 5 M-event window of the
    70/15/15 HTTP / Kafka / Postgres mix, on ONE GPU: the engine picks the global-table K1 (variant 1; the graph is
    beyond the partitioned path's range) and a join table that does not fit LDS.  Row for row against the oracle."""
    from oracle import pyoracle
    c = replay.CONFIGS[5]
    topo = replay.make_topology(c["pods"], c["edges"], replay.SEED_BASE + 5)
    ev, labels = replay.make_events(topo, c["events"], replay.SEED_BASE + 5, mixed=True)
    g = _engine(topo.n_nodes, int(c["edges"] * 1.1), 2, max_labels=128, max_outbound_ips=128, max_window_events=len(ev), max_batch=1 << 20)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    _feed(g, ev, chunk=1 << 20)
    g.set_label_count(len(labels))
    rows = g.flush_window()
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    want = o.edge_rows()
    st = g.stats()
    assert st.events_dropped_cap == 0 and st.last_window_events == o.window_events and len(rows) == len(want) > 2_000_000
    assert st.events_dropped_src == o.dropped_src and st.last_window_nodes == o.n_nodes
    for f in ("from_ref", "to_ref", "count", "err_count", "sum_ns", "max_ns", "sumsq_us", "err_ratio"):
        assert np.array_equal(rows[f], want[f]), f
    assert np.abs(rows["score"] - want["score"]).max() <= 1e-5
    assert (np.abs(rows["lat_z"] - want["lat_z"]) <= 1e-5 * np.maximum(1.0, np.abs(want["lat_z"]))).all()
    pg = ev["protocol"] == replay.PROTO_POSTGRES
    acc = np.isin(ev["saddr"], topo.pod_ips)
    assert int(rows["err_count"].sum()) == int(((ev["status"] >= 500) & acc & (ev["protocol"] == replay.PROTO_HTTP)).sum() + ((ev["status"] == 2) & acc & pg).sum())
    g.close()
    # ... and as config 5 actually runs: the graph hash-sharded by source pod over 8 GPUs.  Eight logical shards on this device,
    # each with the PARTITIONED K1 (variant 0, 8-byte records; 2.75 M-edge capacity per shard, 2048 partitions, join level 2 read
    # from global memory: 150 k replicated IPs do not fit LDS, 18-bit endpoint indices), halo exchange through the real
    # driver — the concatenated rows must equal the one-engine (variant 1) rows above bit for bit.
    from alaz_amd import engine
    probe = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=int(c["edges"] * 1.1) // 8, layers=2, max_labels=128, max_outbound_ips=128,
                                rank=0, world=8, max_window_events=len(ev) // 4)
    geo = probe.geometry(); probe.close()
    assert geo["k1_variant"] == 0 and geo["k1_narrow"] == 1 and geo["endpoint_bits"] >= 18 and geo["partitions"] >= 1024
    got, bad, per = _logical_shards(topo, ev, labels, 2, 8, max_edges=int(c["edges"] * 1.1) // 8)
    assert bad == 0 and min(per) > 200_000
    key = lambda a: np.lexsort((a["to_ref"], a["from_ref"]))
    got = got[key(got)]; exp = rows[key(rows)]
    assert len(got) == len(exp)
    assert got.tobytes() == exp.tobytes()


def test_windows_in_flight_give_the_same_rows_as_one_window_at_a_time():
    """sg_config.windows_in_flight = 3: consecutive windows are closed on their own slots / streams and
    overlap on the device; every window's rows must equal the single-slot engine's, bit for bit."""
    import ctypes
    import torch
    topo = replay.make_topology(100, 1200, seed=111)
    ev, labels = replay.make_events(topo, 120_000, seed=112, mixed=True, with_raw_outbound=True, with_reverse=True)
    wins = [ev[i * 20_000:(i + 1) * 20_000] for i in range(6)]
    ref = _engine(topo.n_nodes + 8, 4096, 2, max_window_events=20_000)
    HostShim().apply(ref, topo.k8s_ops()); ref.set_label_count(len(labels))
    want = []
    for w in wins:
        assert ref.ingest(w) == 0
        want.append(ref.flush_window().copy())
    g = _engine(topo.n_nodes + 8, 4096, 2, max_window_events=20_000, windows_in_flight=3)
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    hip = ctypes.CDLL(None); hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    dev = [torch.from_numpy(w.view(np.uint8).reshape(-1)).cuda() for w in wins]
    torch.cuda.synchronize()
    ptrs = []
    for i, w in enumerate(wins):                      # enqueue all six windows back to back: three slots, used twice each
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        ptrs.append(g.rows_buffer())
        if i >= 3:                                    # slot reuse: the rows of window i-3 are gone, check them before
            pass
    torch.cuda.synchronize()
    assert len(set(ptrs[:3])) == 3 and ptrs[3:] == ptrs[:3]
    for i in (3, 4, 5):                               # the last three windows are still resident in their slots
        n = len(want[i])
        buf = np.zeros(n, dtype=replay.EDGE_OUT_DTYPE)
        assert hip.hipMemcpy(buf.ctypes.data, ctypes.c_void_p(ptrs[i]), n * 64, 2) == 0
        assert buf.tobytes() == want[i].tobytes(), i
    # and the synchronous API keeps working on the current slot
    assert g.ingest(wins[0]) == 0
    assert g.flush_window().tobytes() == want[0].tobytes()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_alive_connections_are_count_only_edges(variant):
    """f-2: SG_EV_ALIVE records (open TCP connections, data.go:1628-1679) go through the same join — no Host
    header, no reversal, a non-pod source is ignored silently — create their edge if the window has no request
    on it, and only add to `alive`.  Edges, accumulators, alive counts, scores (node features 16/17 feed the
    SAGE layers) and the canonical row order must equal the oracle's; two windows, the second without alive
    records, to show the list is re-armed."""
    topo = replay.make_topology(60, 400, seed=91)
    ev, labels = replay.make_events(topo, 30_000, seed=92, with_raw_outbound=True)
    rng = np.random.default_rng(93)
    n_alive = 3000
    al = np.zeros(n_alive, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    src = rng.integers(0, topo.n_pods, n_alive)
    al["saddr"] = topo.pod_ips[src]
    kind = rng.random(n_alive)
    on_edge = rng.integers(0, len(ev), n_alive)
    al["daddr"] = np.where(kind < 0.4, ev["daddr"][on_edge],                                      # where requests also flow
                  np.where(kind < 0.7, topo.svc_ips[rng.integers(0, topo.n_svcs, n_alive)],          # idle service edges
                  np.where(kind < 0.85, topo.pod_ips[rng.integers(0, topo.n_pods, n_alive)],         # pod to pod
                           0x5DB8D800 + rng.integers(0, 40, n_alive)))).astype(np.uint32)            # raw outbound IPs
    al["saddr"][kind < 0.4] = ev["saddr"][on_edge][kind < 0.4]
    al["saddr"][-50:] = 0xC0A80001                                                                   # not a pod: ignored, not counted as dropped
    al["host_label"][::7] = 1                                                                         # must be ignored for alive records
    al["flags"][::11] |= replay.EV_REVERSE                                                            # so must this
    al["duration_ns"] = 12345; al["status"] = 503                                                     # and these
    both = np.concatenate([ev[:15_000], al[:1500], ev[15_000:], al[1500:]])
    ops = topo.k8s_ops()
    g = _engine(topo.n_nodes + 8, 8192, 2, k1_variant=variant, max_window_events=len(both) + 1)
    shim = HostShim(); shim.apply(g, ops)
    o = _oracle(ops, 2)
    W = weights.make_weights(2)
    seen = 0
    for batch, has_alive in ((both, True), (ev[:5000], False)):
        for i in range(0, len(batch), 7001):
            while g.ingest(batch[i:i + 7001]) != 0:          # SG_EAGAIN: staging ring momentarily full -> the test retries
                pass
        g.set_label_count(len(labels))
        rows = g.flush_window()
        o.packed(batch, labels); o.window_close(W, 2)
        want = o.edge_dict()
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), want)
        n_al = sum(v[8] for v in want.values())
        assert int(rows["alive"].sum()) == n_al and (n_al > 2500) == has_alive and (n_al == 0) == (not has_alive)
        seen += n_al
        if has_alive:
            assert sum(1 for v in want.values() if v[0] == 0 and v[8] > 0) > 1000                     # idle edges exist only through alive records
        assert np.array_equal(rows["from_ref"], o.edge_rows()["from_ref"]) and np.array_equal(rows["to_ref"], o.edge_rows()["to_ref"])
        st = g.stats()
        assert st.last_window_events == o.window_events and st.last_window_nodes == o.n_nodes
    assert st.alive_in == seen and st.alive_dropped == 0 and st.events_dropped_src == o.dropped_src


@pytest.mark.parametrize("pods", [2000, 8000, 8738])
def test_join_table_builds_and_resolves_at_full_load(pods):
    """The host-built cuckoo join table at its design load (<= 0.8, e.g. 13107 IPs in 16384 slots) and at the
    sizes the 8-GPU weak-scaling bench uses (12000 IPs): every pod and service IP must resolve — one event per
    (pod, service) pair, and the edge set must be exactly those pairs."""
    from oracle import pyoracle
    topo = replay.make_topology(pods, pods * 2, seed=17)
    n = topo.n_nodes
    ev = np.zeros(n, dtype=replay.EVENT_DTYPE)
    ev["saddr"] = topo.pod_ips[np.arange(n) % topo.n_pods]
    ev["daddr"] = np.concatenate([topo.svc_ips, topo.pod_ips])[np.arange(n) % n]
    ev["protocol"] = replay.PROTO_HTTP; ev["status"] = 200; ev["duration_ns"] = 1000 + np.arange(n); ev["write_time_ns"] = 10**9 + np.arange(n)
    g = _engine(n, n + 1024, 1, max_window_events=n, max_ips=n)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    assert g.ingest(ev) == 0
    rows = g.flush_window()
    st = g.stats()
    assert st.events_dropped_src == 0 and st.last_window_events == n and int(rows["count"].sum()) == n
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, []); o.window_close(weights.make_weights(1), 1)
    compare_edge_dicts(engine_edge_dict(rows, shim, [], g.outbound_ips()), o.edge_dict())


def test_sg_ingest_from_many_threads_into_one_engine():
    """sg_ingest is called from arbitrary OS threads (cgo).  Six threads feed disjoint slices of one window into
    ONE engine through the C ABI (ctypes releases the GIL); the window equals the oracle's, nothing lost or counted twice."""
    import threading
    topo = replay.make_topology(200, 3000, seed=51)
    ev, labels = replay.make_events(topo, 120_000, seed=52, mixed=True, with_raw_outbound=True, with_reverse=True)
    ops = topo.k8s_ops()
    g = _engine(topo.n_nodes + 8, 4 * len(topo.edge_src) + 1024, 2, max_window_events=len(ev) + 1)
    shim = HostShim(); shim.apply(g, ops)
    g.set_label_count(len(labels))
    errs = []
    def feed(part):
        try:
            for i in range(0, len(part), 3001):
                while g.ingest(part[i:i + 3001]) != 0:      # SG_EAGAIN: staging ring momentarily full
                    pass
        except Exception as e:                               # pragma: no cover
            errs.append(e)
    ts = [threading.Thread(target=feed, args=(ev[k::6].copy(),)) for k in range(6)]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs
    rows = g.flush_window()
    o = _oracle(ops, 2); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    st = g.stats()
    assert st.last_window_events == o.window_events and st.events_dropped_cap == 0


def test_k1_path_follows_the_window_size():
    """sg_config.k1_variant = 0: a window of BASELINE config 2's size gets the 16-byte kernels and keeps no state, config 3's the 8-byte
    path with the warm-window state; 3 / SG_CFG_WARM ask for them by name."""
    from alaz_amd import engine
    small = engine.ServiceGraph(max_known_nodes=1600, max_edges=66_000, layers=1, max_window_events=1_000_000)
    g = small.geometry(); small.close()
    assert (g["k1_variant"], g["k1_narrow"], g["warm_windows"]) == (0, 0, 0)
    forced = engine.ServiceGraph(max_known_nodes=1600, max_edges=66_000, layers=1, max_window_events=1_000_000, k1_variant=3, warm=True)
    g = forced.geometry(); forced.close()
    assert (g["k1_narrow"], g["warm_windows"]) == (1, 1)
    big = engine.ServiceGraph(max_known_nodes=15_000, max_edges=1_250_000, layers=2, max_window_events=10_000_000)
    g = big.geometry(); big.close()
    assert (g["k1_narrow"], g["warm_windows"], g["pass_a_teams"]) == (1, 1, 2)


def test_two_concurrent_flushers_beside_eight_feeders_every_window_equals_a_single_flusher():
    """servicegraph.hip flush_begin_locked / flush_end_unlocked: TWO threads close windows at the same time —
    one with sg_flush_window, one with sg_flush_begin + sg_flush_end — while eight feeder threads call sg_ingest, until at least 50
    windows have been closed.  Where a boundary falls is up to the race, so the trace is built to tell afterwards: it is cut into
    chunks with DISJOINT sources (chunk k holds the edges whose source pod is k mod K), each handed over in ONE sg_ingest call,
    which lands in exactly one window.  Then: every chunk appears in exactly one window, whole; every window is byte for byte what a
    single-flusher engine returns for the same chunks; sg_stats.windows counts every close once (no double account_window)."""
    import threading
    import time
    from alaz_amd import engine, sharded
    K, per = 160, 2500
    topo = replay.make_topology(800, 40_000, seed=131)
    nlab = len(replay.EXTERNAL_HOSTS)
    chunks = []
    for k in range(K):
        keep = (topo.edge_src % K) == k
        sub = replay.Topology(topo.n_pods, topo.n_svcs, topo.pod_ips, topo.svc_ips, topo.edge_src[keep], topo.edge_dst[keep], topo.seed)
        ev, _ = replay.make_events(sub, per, seed=500 + k, fixed_labels=True)
        chunks.append(np.ascontiguousarray(ev))
    def mk():
        g = _engine(topo.n_nodes + 8, 1 << 16, 2, max_labels=max(64, nlab), max_window_events=K * per + 1, max_batch=4096)
        HostShim().apply(g, topo.k8s_ops()); g.set_label_count(nlab)
        return g
    a, b = mk(), mk()
    errs, wins, lock = [], [], threading.Lock()
    fed = [0]
    def feed(idx):
        try:
            for k in idx:
                while a.ingest(chunks[k]) != 0:              # SG_EAGAIN: the staging ring is momentarily full
                    pass
                with lock: fed[0] += 1
                time.sleep(0.0005)
        except Exception as ex:                              # noqa: BLE001
            errs.append(ex)
    def done():
        with lock: return fed[0] == K and len(wins) >= 50
    def flusher_one_call():
        try:
            while not done() and not errs:
                r = a.flush_window().copy()
                with lock: wins.append(r)
        except Exception as ex:                              # noqa: BLE001
            errs.append(ex)
    def flusher_two_halves():
        try:
            while not done() and not errs:
                try:
                    a.flush_begin()
                except engine.ServiceGraphError as ex:       # the other flusher's window has not been fetched yet: legitimate, try again
                    if ex.rc != engine.SG_ESTATE: raise
                    continue
                try:
                    r = a.flush_end().copy()
                except engine.ServiceGraphError as ex:       # ... or it fetched ours (one fetch per window, the loser sees the window gone)
                    if ex.rc != engine.SG_ESTATE: raise
                    continue
                with lock: wins.append(r)
        except Exception as ex:                              # noqa: BLE001
            errs.append(ex)
    ths = [threading.Thread(target=feed, args=(list(range(j, K, 8)),)) for j in range(8)]
    ths += [threading.Thread(target=flusher_one_call), threading.Thread(target=flusher_two_halves)]
    for t in ths: t.start()
    for t in ths: t.join()
    assert not errs, errs
    wins.append(a.flush_window().copy())                     # whatever the last boundary left open
    st = a.stats()
    assert st.windows == len(wins) >= 51 and st.events_in == K * per and st.events_dropped_cap == 0 and st.events_dropped_ring == 0
    seen = np.zeros(K, dtype=np.int64)
    nonempty = 0
    for r in wins:
        if not len(r):
            continue
        nonempty += 1
        assert np.all((r["from_ref"] >> 30) == 0)            # sources are pods (known nodes): the id is the pod index
        ks = np.unique((r["from_ref"] & 0x3FFFFFFF) % K)
        seen[ks] += 1
        for k in ks:                                         # the single-flusher engine, the same chunks in one window
            while b.ingest(chunks[int(k)]) != 0:
                pass
        want = b.flush_window()
        assert len(want) == len(r) and want.tobytes() == r.tobytes()
    assert np.all(seen == 1), "a chunk (one sg_ingest call) was split over windows, lost or counted twice"
    assert nonempty >= 5                                     # (the race did cut the stream into several windows)
    a.close(); b.close()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_edge_latency_histogram_and_percentiles(variant):
    """f-3: with SG_CFG_EDGE_HISTOGRAM every edge carries a 16-bin log2 latency histogram and p50 / p99 read off
    it.  Bins and percentiles must equal the oracle's bit for bit — through pass A's cache (16-bit bins per launch, aggregates
    merged across the many small batches of a window), single records (bin from the duration), pass B's table, the CSR
    gather and K5; durations from microseconds to beyond 2^32 ns; alive-only edges report 0.  Everything else in the rows
    must be what the engine reports without the flag."""
    from alaz_amd import engine
    topo = replay.make_topology(120, 1500, seed=131)
    ev, labels = replay.make_events(topo, 150_000, seed=132, mixed=True, with_raw_outbound=True, with_reverse=True)
    rng = np.random.default_rng(133)
    ev = ev.copy()
    ev["duration_ns"] = np.where(rng.random(len(ev)) < 0.02, rng.integers(1, 1 << 36, len(ev)), ev["duration_ns"]).astype(np.uint64)   # tails: < 1 us .. 68 s
    ev["duration_ns"][:2000] = (1 << 17) - 1; ev["duration_ns"][2000:4000] = 1 << 17; ev["duration_ns"][4000:4500] = 1 << 31
    al = np.zeros(500, dtype=replay.EVENT_DTYPE); al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]; al["daddr"] = topo.svc_ips[rng.integers(0, topo.n_svcs, len(al))]
    ev = np.concatenate([ev[:70_000], al, ev[70_000:]])
    ops = topo.k8s_ops()
    W = weights.make_weights(2)
    out = {}
    for hist in (True, False):
        g = _engine(topo.n_nodes + 8, 8192, 2, k1_variant=variant, max_window_events=len(ev) + 1, edge_histogram=hist)
        shim = HostShim(); shim.apply(g, ops)
        for i in range(0, len(ev), 9001):                               # 17 batches: the hot keys' aggregates meet again and again
            while g.ingest(ev[i:i + 9001]) != 0:
                pass
        g.set_label_count(len(labels))
        rows = g.flush_window()
        out[hist] = (rows.copy(), g.window_hist() if hist else None, shim, g.outbound_ips())
        if not hist:
            with pytest.raises(engine.ServiceGraphError):
                g.window_hist()
        assert g.stats().events_dropped_cap == 0
        g.close()
    o = _oracle(ops, 2); o.packed(ev, labels); o.window_close(W, 2)
    rows, hist, shim, obips = out[True]
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, obips), o.edge_dict(), percentiles=True)
    assert np.array_equal(rows["from_ref"], o.edge_rows()["from_ref"]) and np.array_equal(rows["to_ref"], o.edge_rows()["to_ref"])
    want_h = o.edge_hist()
    assert hist.shape == want_h.shape and np.array_equal(hist, want_h)
    assert np.array_equal(hist.sum(axis=1), rows["count"]) and (hist[:, 0].sum() > 1500) and (hist[:, 15].sum() >= 400)
    assert int((rows["count"] == 0).sum()) > 0 and not rows["p50_us"][rows["count"] == 0].any()
    assert (rows["p50_us"] <= rows["p99_us"]).all() and (rows["p99_us"].astype(np.uint64) * 1000 <= rows["max_ns"]).all()
    plain = out[False][0]
    for f in plain.dtype.names:
        if f not in ("p50_us", "p99_us"):
            assert np.array_equal(plain[f], rows[f]), f
    assert not plain["p50_us"].any() and not plain["p99_us"].any()


def test_edge_histogram_at_config2_scale():
    """Config 2 at full size with the histogram on: bins against numpy (every accepted event lands in exactly one bin of
    its edge: column sums = the trace's bin counts), row for row against the oracle."""
    topo, ev, labels, L = replay.make_config(2)
    g = _engine(topo.n_nodes + 8, 1 << 16, L, max_window_events=len(ev) + 1, edge_histogram=True)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    _feed(g, ev)
    g.set_label_count(len(labels))
    rows = g.flush_window(); hist = g.window_hist()
    acc = np.isin(ev["saddr"], topo.pod_ips)
    assert np.array_equal(hist.sum(axis=0), np.bincount(replay.hist_bin(ev["duration_ns"][acc]), minlength=16))
    o = _oracle(topo.k8s_ops(), L); o.packed(ev, labels); o.window_close(weights.make_weights(L), L)
    want = o.edge_rows()
    for f in ("from_ref", "to_ref", "count", "sum_ns", "max_ns", "p50_us", "p99_us"):
        assert np.array_equal(rows[f], want[f]), f
    assert np.array_equal(hist, o.edge_hist()) and g.stats().events_dropped_cap == 0


def test_join_table_churn_at_150k_ips_with_windows_in_flight():
    """pod / service churn at config-5 table size (100 k pods + 50 k services = 150 k IPs) while four
    windows are in flight.  Between every 50 k-event batch the tables change (new pods in old and in new /24s, deleted pods,
    pods that move to another IP, a service that appears and goes) — in the reference that is one map write per k8s event
    (aggregator/persist.go:55-71, 114-130), here a few table words shipped in stream order.  Every window must equal the
    oracle that saw the same operations at the same points of the stream, the device copy must never be replaced as a whole
    after the initial upload, and a churned window must not cost more than twice a quiet one."""
    import time
    from alaz_amd import engine
    from oracle import pyoracle
    P, S = 100_000, 50_000
    topo = replay.make_topology(P, 300_000, seed=171, svcs=S)
    ev, labels = replay.make_events(topo, 8 * 200_000, seed=172)
    ops0 = topo.k8s_ops()
    g = _engine(topo.n_nodes + 4096, 600_000, 1, max_window_events=200_000, windows_in_flight=4, max_ips=topo.n_nodes + 4096)
    shim = HostShim(); shim.apply(g, ops0)
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(ops0)
    W = weights.make_weights(1)
    g.set_label_count(len(labels))
    rng = np.random.default_rng(173)
    next_new = [0]

    def churn():
        ops = []
        for _ in range(12):                                          # new pods: half in the pods' own /24s' neighbourhood, half far away
            k = next_new[0]; next_new[0] += 1
            ip = int(topo.pod_ips[-1]) + 1 + k if k % 2 == 0 else engine.ip_u32("172.31.0.0") + 37 * k
            ops.append(("pod", "ADD", f"churn-pod-{k}", replay.ip_str(ip)))
        for _ in range(8):                                           # deleted pods (their events are dropped from now on)
            i = int(rng.integers(0, P)); ops.append(("pod", "DELETE", topo.pod_uid(i), replay.ip_str(int(topo.pod_ips[i]))))
        for _ in range(4):                                           # a pod gets a second IP (UPDATE adds, the old key stays: persist.go:55-71)
            i = int(rng.integers(0, P)); k = next_new[0]; next_new[0] += 1
            ops.append(("pod", "UPDATE", topo.pod_uid(i), replay.ip_str(engine.ip_u32("172.30.0.0") + 11 * k)))
        j = int(rng.integers(0, S))
        ops.append(("svc", "DELETE", topo.svc_uid(j), replay.ip_str(int(topo.svc_ips[j]))))
        ops.append(("svc", "ADD", f"churn-svc-{next_new[0]}", replay.ip_str(int(topo.svc_ips[j]))))   # the ClusterIP is taken over
        return ops

    def window(e, with_churn):
        dt = 0.0                                                     # engine time only (table calls, ingest, flush)
        for i in range(0, len(e), 50_000):
            b = e[i:i + 50_000].copy()
            ops = churn() if with_churn else []
            if ops:
                new_ips = [engine.ip_u32(ip) for k, et, _, ip in ops if k == "pod" and et != "DELETE"]
                b["saddr"][:len(new_ips)] = new_ips                  # the new addresses are used at once
            t0 = time.perf_counter()
            shim.apply(g, ops)
            rc = g.ingest(b)
            while rc != 0:
                rc = g.ingest(b)
            dt += time.perf_counter() - t0
            o.apply_ops(ops); o.packed(b, labels)
        t0 = time.perf_counter()
        rows = g.flush_window()
        dt += time.perf_counter() - t0
        o.window_close(W, 1)
        compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
        assert g.stats().last_window_events == o.window_events
        return dt

    wins = [ev[i * 200_000:(i + 1) * 200_000] for i in range(8)]
    window(wins[0], False)                                            # warm-up (first upload)
    full0 = g.stats().join_full_uploads
    quiet = min(window(wins[1], False), window(wins[2], False))
    churned = [window(w, True) for w in wins[3:8]]
    st = g.stats()
    assert st.join_full_uploads == full0, "a table change replaced the whole device copy"
    assert st.join_word_updates > 0
    assert g.stats().events_dropped_src == o.dropped_src
    assert min(churned) < 2.0 * quiet + 0.01, (quiet, churned)


def test_config5_stream_of_raw_records_at_the_nominal_rate_loses_nothing():
    """BASELINE config 5 as it would run in production (tools/c5_stream.py): raw 1096-byte l7_event records of the 70/15/15
    HTTP / Kafka / Postgres mix, eight feeder threads -> C++ GraphDS::IngestWire (payload parse, interning, packing,
    per-thread batches) -> sg_ingest, one engine with 100 k pods + 50 k services and the 20 M-edge variant-1 tables, a
    dispatcher closing a window every second; the records are expanded on the fly by the C++ feeders from 8 M packed events drawn
    from the 20 M-edge graph.  At the nominal 5 M events/s: nothing dropped by the staging ring, by capacity or by the host
    batches, every window closes well inside its second and carries more than 2 M distinct edges.
    (The correctness of such a window against the oracle is the full-size C5 test above.)"""
    import json, subprocess, sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "c5_stream.py")
    out = subprocess.run([sys.executable, tool, "--rate", "5e6", "--windows", "3"], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert lines, out.stderr[-2000:]
    r = json.loads(lines[-1])
    assert r["events_dropped_ring"] == 0 and r["events_dropped_cap"] == 0 and r["host_batches_dropped"] == 0 and r["engine_errors"] == 0
    assert r["engine_events_per_s"] >= 4.9e6, r
    assert r["window_close_ms"]["max"] < 800.0, r
    assert r["rows_per_window"]["min"] > 2_000_000, r               # the stream touches millions of the graph's 20 M edges per window


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_small_windows_against_the_oracle(seed):
    """Randomised sweep over what the big tests fix: graph size (5..400 pods), events per window (0..30 k), batch raggedness,
    SAGE depth, both K1 variants, the histogram flag, alive records, raw-IP / Host-label destinations, reversal, table
    changes between the windows — three windows each, every window row for row against the oracle."""
    from alaz_amd import engine
    rng = np.random.default_rng(9000 + seed)
    pods = int(rng.integers(5, 400)); edges = int(rng.integers(pods, min(pods * 12, pods * (pods + pods // 2 - 1)) + 1))
    layers = 1 + seed % 2; variant = (seed // 2) % 3; hist = (seed // 6) % 2 == 1
    topo = replay.make_topology(pods, edges, seed=9100 + seed)
    ops = topo.k8s_ops()
    g = _engine(topo.n_nodes + 64, 1 << 14, layers, k1_variant=variant, max_window_events=40_000, edge_histogram=hist)
    shim = HostShim(); shim.apply(g, ops)
    o = _oracle(ops, layers)
    W = weights.make_weights(layers)
    lab_all = []
    for w in range(3):
        n = int(rng.integers(0, 30_000)) if w else int(rng.integers(1, 30_000))
        ev, labels = replay.make_events(topo, n, seed=9200 + 10 * seed + w, mixed=True, with_raw_outbound=True, with_reverse=True, stream_base=1000 * w)
        remap = np.zeros(len(labels) + 1, dtype=np.uint32)
        for i, s in enumerate(labels):
            if s not in lab_all: lab_all.append(s)
            remap[i + 1] = lab_all.index(s) + 1
        ev = ev.copy(); ev["host_label"] = remap[ev["host_label"]]
        if n > 10:
            k = int(rng.integers(1, min(n, 200)))
            ev["duration_ns"][:k] = rng.integers(1, 1 << 36, k).astype(np.uint64)                       # sub-microsecond .. 68 s
            al = np.zeros(int(rng.integers(0, 50)), dtype=replay.EVENT_DTYPE); al["flags"] = replay.EV_ALIVE
            al["saddr"] = topo.pod_ips[rng.integers(0, topo.n_pods, len(al))]
            al["daddr"] = np.concatenate([topo.svc_ips, topo.pod_ips])[rng.integers(0, topo.n_nodes, len(al))]
            ev = np.concatenate([ev[: n // 2], al, ev[n // 2:]])
        if w == 1:                                                   # the tables move between the windows
            i = int(rng.integers(0, pods)); j = int(rng.integers(0, topo.n_svcs))
            chg = [("pod", "DELETE", topo.pod_uid(i), replay.ip_str(int(topo.pod_ips[i]))),
                   ("pod", "ADD", f"late-pod-{seed}", "10.250.%d.%d" % (seed, 1 + i % 250)),
                   ("svc", "UPDATE", topo.svc_uid(j), "10.251.%d.7" % seed)]
            shim.apply(g, chg); o.apply_ops(chg)
            if len(ev): ev["saddr"][: max(1, len(ev) // 50)] = engine.ip_u32("10.250.%d.%d" % (seed, 1 + i % 250))
        pos = 0
        while pos < len(ev):                                         # ragged batches
            step = int(rng.integers(1, 9000))
            while g.ingest(ev[pos:pos + step]) != 0:
                pass
            pos += step
        g.set_label_count(len(lab_all))
        rows = g.flush_window()
        o.packed(ev, lab_all); o.window_close(W, layers)
        compare_edge_dicts(engine_edge_dict(rows, shim, lab_all, g.outbound_ips()), o.edge_dict(), percentiles=hist)
        want = o.edge_rows()
        assert np.array_equal(rows["from_ref"], want["from_ref"]) and np.array_equal(rows["to_ref"], want["to_ref"])
        st = g.stats()
        assert st.last_window_events == o.window_events and st.events_dropped_cap == 0 and st.events_dropped_src == o.dropped_src
        if hist and len(rows):
            assert np.array_equal(g.window_hist(), o.edge_hist())
    g.close()


def test_ingest_pinned_reads_registered_caller_memory_without_the_staging_copy():
    """sg_host_register + sg_ingest_pinned: the same window fed half through sg_ingest (staging copy) and half straight out of
    registered caller memory, from two threads, equals the oracle; events outside registered memory are refused."""
    import threading
    from alaz_amd import engine
    topo = replay.make_topology(300, 4000, seed=4401)
    ev, labels = replay.make_events(topo, 120_000, seed=4402, mixed=True, with_raw_outbound=True, with_reverse=True)
    ev = np.ascontiguousarray(ev)
    g = _engine(topo.n_nodes + 8, 1 << 15, 2, max_window_events=len(ev) + 1, max_batch=1 << 14)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    with pytest.raises(engine.ServiceGraphError):
        g.ingest_pinned(ev[:100])                                    # not registered
    g.host_register(ev)
    half = len(ev) // 2

    def feed(part, put):
        for j in range(0, len(part), 1 << 14):
            while put(part[j:j + (1 << 14)]) != 0:
                pass
    third = half // 2
    assert g.ingest_bulk(ev[:third]) >= 0                            # the blocking convenience form, pageable memory
    ths = [threading.Thread(target=feed, args=(ev[third:half], g.ingest)), threading.Thread(target=feed, args=(ev[half:], g.ingest_pinned))]
    for t in ths: t.start()
    for t in ths: t.join()
    g.set_label_count(len(labels))
    rows = g.flush_window()
    g.host_unregister(ev)
    o = _oracle(topo.k8s_ops(), 2); o.packed(ev, labels); o.window_close(weights.make_weights(2), 2)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    assert g.stats().last_window_events == o.window_events
    g.close()


def test_histogram_engine_at_config3_geometry_with_many_ip_blocks():
    """with SG_CFG_EDGE_HISTOGRAM the 16-byte pass A has 72-byte cache slots; at a C3-sized edge capacity
    (4096 partitions) and more than ~90 populated /24 blocks, level 2 of the join no longer fits LDS and the fallback used to ask
    for more than a CU's 160 KiB — every sg_ingest failed with SG_ENODEV.  The geometry now takes the largest cache that fits:
    ingest works, nothing is dropped, rows and bins equal the oracle."""
    topo = replay.make_topology(600, 9000, seed=5151)
    # one /24 block per pod and per service: 900 level-2 blocks (900 KiB of level 2: far beyond LDS)
    pod_ips = (0x0A000000 + np.arange(topo.n_pods) * 256 + 7).astype(np.uint32)
    svc_ips = (0xAC100000 + np.arange(topo.n_svcs) * 256 + 9).astype(np.uint32)
    topo = replay.Topology(topo.n_pods, topo.n_svcs, pod_ips, svc_ips, topo.edge_src, topo.edge_dst, topo.seed)
    ev, labels = replay.make_events(topo, 200_000, seed=5152, mixed=True)
    g = _engine(topo.n_nodes + 8, 1_300_000, 1, max_window_events=len(ev) + 1, edge_histogram=True, max_batch=1 << 16,
                max_ips=32_768)                                         # room for 1024 /24 blocks (the engine allows max_ips / 32)
    geo = g.geometry()
    assert geo["k1_narrow"] == 0 and geo["partitions"] >= 2048          # the histogram rides the 16-byte kernels
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    for i in range(0, len(ev), 1 << 16):
        assert g.ingest(ev[i:i + (1 << 16)]) == 0, g.geometry()
    assert g.geometry()["join_l2_in_lds"] == 0                          # 900 blocks: level 2 is read from global memory
    g.set_label_count(len(labels))
    rows = g.flush_window()
    hist = g.window_hist()
    o = _oracle(topo.k8s_ops(), 1); o.packed(ev, labels); o.window_close(weights.make_weights(1), 1)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict(), percentiles=True)
    assert np.array_equal(hist, o.edge_hist()) and g.stats().events_dropped_cap == 0
    g.close()


# ---- the RCCL entry point (sg_window_run_sharded): rows checked, not just timed -------------------------------
def _rccl_rank(rank, world, idfile, outdir, layers):
    """One rank of the sharded window through the library's own RCCL communicator (also the body of the world = 1 test).
    The unique id travels through a file (no torch.distributed in the picture: the C ABI is all a Go / C++ host has)."""
    import time
    import torch
    from alaz_amd import engine
    topo = replay.make_topology(300, 6000, seed=171)
    ev, labels = replay.make_events(topo, 200_000, seed=172, mixed=True, with_raw_outbound=True, with_reverse=True, fixed_labels=True)
    torch.cuda.set_device(rank)

    def bcast(raw):
        if rank == 0:
            with open(idfile + ".tmp", "wb") as f: f.write(raw)
            os.replace(idfile + ".tmp", idfile)
            return raw
        t0 = time.time()
        while not os.path.exists(idfile):
            if time.time() - t0 > 120: raise RuntimeError("no unique id from rank 0")
            time.sleep(0.01)
        return open(idfile, "rb").read()
    comm = engine.RcclComm(rank, world, rank, bcast)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=16384, layers=layers, max_labels=128, max_outbound_ips=512,
                            device=rank, rank=rank, world=world, max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(layers))
    shim = HostShim(); shim.apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    mine = ev[g.route(ev, world) == rank] if world > 1 else ev
    st = torch.cuda.Stream(torch.device("cuda", rank))
    dev = torch.from_numpy(mine.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", rank))
    outs = []
    for _ in range(2):                                               # two windows through the same engine and communicator
        g.ingest_device(dev.data_ptr(), len(mine), st.cuda_stream)
        g.window_run_sharded(comm, st.cuda_stream)
        outs.append(g.window_read().copy())
    assert outs[0].tobytes() == outs[1].tobytes()
    s = g.stats()
    assert s.events_dropped_cap + s.events_misrouted + s.halo_overflow == 0
    np.save(os.path.join(outdir, f"rows_{rank}.npy"), outs[0]); np.save(os.path.join(outdir, f"obips_{rank}.npy"), g.outbound_ips())
    comm.close(); g.close()


def _rccl_check(outdir, world, layers):
    from oracle import pyoracle
    topo = replay.make_topology(300, 6000, seed=171)
    ev, labels = replay.make_events(topo, 200_000, seed=172, mixed=True, with_raw_outbound=True, with_reverse=True, fixed_labels=True)
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(weights.make_weights(layers), layers)
    rows = np.concatenate([np.load(os.path.join(outdir, f"rows_{r}.npy")) for r in range(world)])
    obips = np.load(os.path.join(outdir, "obips_0.npy"))
    assert all(np.array_equal(obips, np.load(os.path.join(outdir, f"obips_{r}.npy"))) for r in range(world))   # identical node numbering everywhere
    shim = HostShim()
    for kind, et, uid, ip in topo.k8s_ops():
        if not (kind == "pod" and ip == ""): shim.intern(uid, "pod" if kind == "pod" else "service")
    got = engine_edge_dict(rows, shim, labels, obips)
    assert len(got) == len(rows)                                     # no edge on two shards
    assert compare_edge_dicts(got, o.edge_dict()) <= 1e-5
    assert np.array_equal(obips, o.outbound_ips())


@pytest.mark.parametrize("layers", [2])
def test_rccl_entry_point_world1_rows_against_the_oracle(layers, tmp_path):
    """sg_comm_create + sg_window_run_sharded at world = 1 (what `bench.py` under SG_FORCE_SHARDED times): the staged pipeline with the
    collectives issued on RCCL from inside the library — rows row for row against the oracle, two windows."""
    _rccl_rank(0, 1, str(tmp_path / "id"), str(tmp_path), layers)
    _rccl_check(str(tmp_path), 1, layers)


def test_rccl_entry_point_two_ranks_rows_against_the_oracle(tmp_path):
    """The same with two processes on two GPUs (grouped ncclSend / ncclRecv all-to-all, all-gather, all-reduce over xGMI): the
    concatenated rows of the two shards against the oracle.  Skipped on a one-GPU box."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_rccl_rank, args=(r, 2, str(tmp_path / "id"), str(tmp_path), 2)) for r in range(2)]
    for p in ps: p.start()
    for p in ps: p.join(timeout=600)
    assert all(p.exitcode == 0 for p in ps)
    _rccl_check(str(tmp_path), 2, 2)


def test_config5_one_shard_of_eight_the_bench_engine_row_for_row():
    """BASELINE config 5 as it is specified — hash-sharded over 8 GPUs — seen from ONE shard, with the engine exactly as
    `bench.py --config 5 --shard-of 8` builds it (sg_create's own K1 rule for a 150 k-node, ~440 k-edge shard: the 8-byte records with
    18-bit endpoints, 1024 partitions, level 2 of the join read from global memory, and — round 6 — pass A as k1a_team_partition with the
    16-lanes-per-run copy-out): one 625 k-event window of the mixed HTTP / Kafka / Postgres stream against the oracle row for row (until
    round 5 a tool, tools/c5_shard_check.py)."""
    from alaz_amd import engine, sharded
    from oracle import pyoracle
    c = replay.CONFIGS[5]; seed = replay.SEED_BASE + 5
    full = replay.make_topology(c["pods"], c["edges"], seed)
    topo = sharded.shard_view(full, 0, 8)
    Ev = c["events"] // 8
    ev, labels = replay.make_events(topo, Ev, seed, mixed=True)
    L = c["layers"]
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=int(min(len(topo.edge_src), Ev) * 1.25) + 4096, layers=L,
                            max_labels=max(64, len(labels)), max_outbound_ips=64, max_batch=1 << 20, max_window_events=Ev, warm=False)
    geo = g.geometry()
    assert geo["k1_narrow"] == 1 and geo["endpoint_bits"] >= 18 and geo["pass_a_teams"] == 2, geo
    g.set_clock(*CLOCK); W = weights.make_weights(L); g.load_weights(W)
    shim = HostShim(); shim.apply(g, topo.k8s_ops())
    g.set_label_count(len(labels))
    for _ in range(2):                                               # (a second window over the first one's pieces: the headers carry over)
        for i in range(0, len(ev), 1 << 18):
            while g.ingest(ev[i:i + (1 << 18)]) != 0:
                pass
        rows = g.flush_window().copy()
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops()); o.packed(ev, labels); o.window_close(W, L)
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, g.outbound_ips()), o.edge_dict())
    orow = o.edge_rows()
    assert np.array_equal(rows["from_ref"], orow["from_ref"]) and np.array_equal(rows["to_ref"], orow["to_ref"])
    assert g.stats().events_dropped_cap == 0
    g.close()
