"""K3's node statistics and features and K4's layer outputs read from the device and held to references (tests/model_ref.py), stage by
stage: after sg_window_close the statistics equal the oracle's and a recount word for word; after sg_window_features x0 is within 1 fp32
ulp of the oracle and of the float64 reference; with the oracle's x0 copied over the device's, every sg_window_layer output equals the
oracle's layer output BYTE FOR BYTE (the pinned summation order), all 64 units of every node; the rows after
sg_window_score equal the oracle's.  The one-call pipelines (sg_flush_window, sg_window_run: the fused in-sum, the layer kernels that
also project) leave the same x0 and h[l] as the staged one.  On the adversarial trace and on model_ref.boundary_trace, for every K1
variant, both depths, both dense paths, both K4 forms, slice counts that hit every tail loop, a warm engine, node capacities beyond
one trip of the K4 tiles (32 768) and of k3_node_features (262 144), and over buffers filled with NaN."""

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.gpu_model_scaffold import C_COUNT, C_N_NODES, TRACES, _sync, bits, check_rows, check_stats, check_x0, dev_read, dev_write, knobs, oracle, trace
from tests.helpers import CLOCK, HostShim
from tests import model_ref as mr

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------
# device memory
# ------------------------------------------------------------------------------------------------


class Eng:
    """an engine on trace `name` under make_weights(layers), with its statistics, counter and feature buffers"""

    def __init__(self, name, layers, variant=3, **kw):
        from alaz_amd import engine
        topo, ev, labels = trace(name)
        kw.setdefault("max_edges", TRACES[name][1])
        self.g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, layers=layers, max_labels=128, max_outbound_ips=512,
                                     k1_variant=variant, max_window_events=len(ev) + 1, **kw)
        self.g.set_clock(*CLOCK)
        HostShim().apply(self.g, topo.k8s_ops()); self.g.set_label_count(len(labels))
        self.g.load_weights(weights.make_weights(layers))
        self.layers = layers
        self.attach()

    def attach(self):
        self.sum, self.max, self.ctr, self.ncap = self.g.window_buffers()
        self.feat = [self.g.feat_buffer(l) for l in range(self.layers + 1)]
        assert [w for _, w in self.feat] == [mr.F_IN] + [mr.F_HID] * self.layers
        return self

    def n_nodes(self):
        return int(dev_read(self.ctr, (C_COUNT,), np.uint64)[C_N_NODES])

    def stats(self):
        return dev_read(self.sum, (self.ncap, mr.SUM_WORDS), np.uint64), dev_read(self.max, (self.ncap, mr.MAX_WORDS), np.uint64)

    def rows(self, l):
        """x0 (l = 0) or h[l], the whole capacity"""
        return dev_read(self.feat[l][0], (self.ncap, self.feat[l][1]), np.float32)

    def fill_nan(self):
        for p, w in self.feat:
            dev_write(p, np.full((self.ncap, w), np.nan, dtype=np.float32))

    def close(self):
        _sync(); self.g.close()


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------


def check_layer_bound(hin, hout, o, l, tag):
    """the device's layer l output against the float64 layer of the device's own input: every element within the derived bound"""
    assert np.isfinite(hout).all(), tag
    ref, bound = mr.sage_layer_ref(hin, *o["csr"], *mr.layer_weights(o["w"], l))
    err = np.abs(hout.astype(np.float64) - ref)
    assert np.all(err <= bound), (tag, l, np.argwhere(err > bound)[:4].tolist(), float(np.max(err / bound)))


def check_equals_oracle(h, o, l, tag):
    want = o["h"][l]
    bad = np.argwhere(bits(h) != bits(want))
    assert len(bad) == 0, (f"{tag}: h[{l}] differs from the oracle's on {len(bad)} elements of {len(np.unique(bad[:, 0]))} nodes", bad[:4].tolist(),
                           [float(h[tuple(b)]) for b in bad[:2]], [float(want[tuple(b)]) for b in bad[:2]])


def staged(E, name, tag, through_score=True):
    """one window of the trace through the staged calls with every check of the module docstring; -> the device's own x0 and h[1..L]
    (computed WITHOUT the oracle's x0 copied in) and whether that x0 is bit-equal to the oracle's"""
    o = oracle(name, E.layers)
    g, N, L = E.g, o["n"], E.layers
    assert N <= E.ncap
    assert g.ingest(trace(name)[1]) == 0
    g.window_close()
    check_stats(E, o, tag)
    g.window_features()
    x0 = E.rows(0)[:N].copy()
    same = check_x0(x0, o, tag)
    h = [x0]
    for l in range(L):                                               # the layers of the device's own x0
        g.window_layer(l)
        h.append(E.rows(l + 1)[:N].copy())
        check_layer_bound(h[l], h[l + 1], o, l, tag)
    dev_write(E.feat[0][0], o["x0"])                                  # a bit-pattern copy: K4 alone from here on
    for l in range(L):
        g.window_layer(l)
        check_equals_oracle(E.rows(l + 1)[:N], o, l + 1, tag)
    if through_score:
        g.window_score()
        rows = g.window_read().copy()
        g.window_reset()
        check_rows(rows, o["rows"], tag)
    return dict(h=h, same=same)


def one_call(name, layers, how, st, tag, variant=3, **kw):
    """the same window through sg_flush_window / sg_window_run on a twin engine: x0 and every h[l] equal the staged pipeline's byte for
    byte, the rows the oracle's; where the staged x0 is the oracle's bit for bit, every h[l] is the oracle's too"""
    o = oracle(name, layers)
    N = o["n"]
    E = Eng(name, layers, variant, **kw)
    try:
        assert E.g.ingest(trace(name)[1]) == 0
        if how == "flush_window":
            rows = E.g.flush_window().copy()
        else:
            E.g.window_run()
            rows = dev_read(E.g.rows_buffer(), (len(o["rows"]),), replay.EDGE_OUT_DTYPE)
        E.attach()
        check_rows(rows, o["rows"], f"{tag} {how}")
        for l in range(layers + 1):
            got = E.rows(l)[:N]
            bad = np.argwhere(bits(got) != bits(st["h"][l]))
            assert len(bad) == 0, (f"{tag} {how}: {'x0' if l == 0 else f'h[{l}]'} differs from the staged pipeline's on {len(bad)} elements", bad[:4].tolist())
            if st["same"] and l:
                check_equals_oracle(got, o, l, f"{tag} {how} (chain)")
    finally:
        E.close()


def suite(name, layers, tag, variant=3, hows=("flush_window", "window_run"), **kw):
    E = Eng(name, layers, variant, **kw)
    try:
        st = staged(E, name, tag)
    finally:
        E.close()
    if name == "adversarial":
        assert st["same"], f"{tag}: the device's x0 is not bit-equal to the oracle's on the adversarial trace"
    for how in hows:
        one_call(name, layers, how, st, tag, variant, **kw)
    return st


# ------------------------------------------------------------------------------------------------
# the shipped library
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("name", ["adversarial", "boundary"])
def test_every_stage_on_every_k1_variant(name, layers, variant):
    suite(name, layers, f"{name} L={layers} variant {variant}", variant)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("name", ["adversarial", "boundary"])
def test_every_stage_with_the_gather_launch_of_large_engines(name, layers):
    """an edge capacity above 2^17: the shipped library's k4_gather + PRE tiles (hub work items, block sums eight at a time), 16 slices"""
    suite(name, layers, f"{name} L={layers} split", max_edges=(1 << 17) + 4096)


# ------------------------------------------------------------------------------------------------
# the development build's knobs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valu", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_every_stage_on_both_dense_paths_and_both_k4_forms(valu, fused):
    """MFMA and VALU dense tiles, one fused launch and gather + tiles: all of k4_layer[wide][pj] with and without k4_gather"""
    with knobs(SG_DENSE_VALU=valu, SG_K4_FUSED=fused):
        for name in ("adversarial", "boundary"):
            for layers in (1, 2):
                suite(name, layers, f"{name} L={layers} valu={valu} fused={fused}", dev_knobs=True)


@pytest.mark.parametrize("slices", [1, 5, 33, 47, 48])
def test_every_stage_at_slice_counts_that_hit_every_tail_loop(slices):
    """k3_in_part's slices on the boundary trace: 1 = a scan of several 8 192-edge trips; 5, 33 and 47 = the tail loops of k3_in_reduce
    (eight at a time, staged) and of k3_node_features' own sum (four at a time, one call); 48 = the largest plan value"""
    with knobs(SG_K3_SLICES=slices):
        suite("boundary", 2, f"boundary L=2 slices={slices}", hows=("flush_window",), dev_knobs=True)


@pytest.mark.parametrize("name", ["adversarial", "boundary"])
def test_one_call_pipelines_without_the_fused_in_sum(name):
    """SG_K3_NO_FUSE=1: the one-call pipelines launch k3_in_reduce as the staged one does"""
    with knobs(SG_K3_NO_FUSE=1):
        suite(name, 2, f"{name} L=2 no-fuse", dev_knobs=True)


# ------------------------------------------------------------------------------------------------
# warm windows, stale buffers
# ------------------------------------------------------------------------------------------------
def test_warm_windows_give_the_same_statistics_features_and_layers():
    """a warm engine (kw_finish_rows writes the out-statistics and the hub work items instead of the row sort): the second and third
    window of the boundary trace without raw outbound IPs pass every staged check and equal the first window's x0 and h"""
    name, L = "boundary_known", 2
    E = Eng(name, L, warm=True)
    try:
        first = staged(E, name, "warm window 1")
        for i in (2, 3):
            w0 = E.g.stats().windows_warm
            st = staged(E.attach(), name, f"warm window {i}")
            assert E.g.stats().windows_warm == w0 + 1, "the window did not take the warm path"
            for l in range(L + 1):
                assert np.array_equal(bits(st["h"][l]), bits(first["h"][l])), (i, l)
    finally:
        E.close()


def test_stale_rows_do_not_reach_a_window():
    """x0 and every h[l] filled with NaN over the whole capacity before each of three windows (the boundary trace, every second event of
    it, the boundary trace again): rows [:N] are written anew, the scores equal the oracle's"""
    L = 2
    E = Eng("boundary", L)
    try:
        for i, name in enumerate(("boundary", "boundary_half", "boundary")):
            o = oracle(name, L)
            N = o["n"]
            E.attach().fill_nan()
            assert E.g.ingest(trace(name)[1]) == 0
            rows = E.g.flush_window().copy()
            tag = f"window {i} ({name}) over NaN"
            check_rows(rows, o["rows"], tag)
            h = [E.attach().rows(l)[:N] for l in range(L + 1)]
            same = check_x0(h[0], o, tag)
            for l in range(L):
                check_layer_bound(h[l], h[l + 1], o, l, tag)
                if same:
                    check_equals_oracle(h[l + 1], o, l + 1, tag)
    finally:
        E.close()


# ------------------------------------------------------------------------------------------------
# second trips
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [None, "0"])
def test_second_trip_of_the_k4_tiles_above_32768_nodes(fused):
    """a node capacity of 33 712: the tile loop of k4_sage_layer (2 048 workgroups x 16 rows) and k4_gather's grid (8 192 x 4 rows, the
    development build's SG_K4_FUSED=0) take a second trip; out-rows and in-edges on both sides of node 32 768, L = 2"""
    name = "sparse33k"
    o = oracle(name, 2)
    assert (o["u"] >= 32768).sum() > 100 and (o["v"] >= 32768).sum() > 100 and (o["u"] < 32768).any() and (o["v"] < 32768).any()
    with knobs(**({} if fused is None else {"SG_K4_FUSED": fused})):
        E = Eng(name, 2, dev_knobs=fused is not None)
        try:
            assert E.ncap > 32768 + 16
            staged(E, name, f"{name} fused={fused}")
        finally:
            E.close()


def test_second_trip_of_the_node_features_above_262144_nodes():
    """a node capacity of 262 480: k3_node_features' node loop (2 048 workgroups x 128 nodes) takes a second trip.  Statistics and x0
    against node_stats_ref / node_features_ref of the engine's own rows (the oracle is not closed at this size)"""
    from alaz_amd import engine
    NP = 262_400
    topo, ev, _ = mr.sparse_trace(NP, 262_100, 4000, seed=0x5A26, n_svcs=0)
    g = engine.ServiceGraph(max_known_nodes=NP, max_edges=8192, layers=1, max_labels=16, max_outbound_ips=64, max_window_events=len(ev) + 1)
    try:
        g.set_clock(*CLOCK)
        speak = np.unique(np.concatenate([ev["saddr"], ev["daddr"], topo.pod_ips[-1:]]).astype(np.int64) - replay.POD_IP_BASE)
        for i in speak:
            g.upsert_pod(int(topo.pod_ips[i]), int(i))
        g.load_weights(weights.make_weights(1))
        a, b, c, ncap = g.window_buffers()
        assert ncap > 262144 + 128
        assert g.ingest(ev) == 0
        g.window_close()
        s = dev_read(a, (ncap, mr.SUM_WORDS), np.uint64); m = dev_read(b, (ncap, mr.MAX_WORDS), np.uint64)
        N = int(dev_read(c, (C_COUNT,), np.uint64)[C_N_NODES])
        assert N == NP
        g.window_features()
        x0 = dev_read(g.feat_buffer(0)[0], (ncap, mr.F_IN), np.float32)[:N]
        g.window_layer(0); g.window_score()
        rows = g.window_read().copy()
        g.window_reset()
        assert len(rows) > 3000 and not (rows["from_ref"] >> 30).any() and not (rows["to_ref"] >> 30).any()
        u, v = rows["from_ref"].astype(np.int64), rows["to_ref"].astype(np.int64)
        assert (u >= 262144).sum() > 100 and (v >= 262144).sum() > 100 and (u < 262144).any() and (v < 262144).any()
        rs, rm = mr.node_stats_ref(rows, N, u, v)
        assert np.array_equal(s[:N], rs) and np.array_equal(m[:N], rm)
        assert not s[N:].any() and not m[N:].any()
        kind = np.zeros(N, dtype=np.uint8); kind[speak] = mr.NODE_POD
        d = mr.ulp_distance(x0, mr.node_features_ref((rs, rm), kind))
        print(f"262 400 nodes: {int((d != 0).sum())} of {d.size} elements of x0 are not bit-equal to the float64 reference (max {int(d.max())} ulp)")
        assert d.max() <= 1, np.argwhere(d > 1)[:4].tolist()
        assert np.all(bits(x0[:, 18:]) == 0) and np.all(x0[:, 15] == 1.0)
    finally:
        _sync(); g.close()
