"""Probe blobs on the CPU oracle (tests/probe_weights.py): under each blob the recovered phi equals the oracle's own node features,
layer outputs and a float64 restatement of the edge features, within the readout bound that tests/test_gpu_probe.py reuses.  No GPU."""
import numpy as np
import pytest

from tests.helpers import CLOCK
from tests import probe_weights as pw


@pytest.fixture(scope="module")
def trace():
    return pw.adversarial_trace()


def _oracle(oracle_lib, trace):
    topo, ev, labels = trace
    o = oracle_lib.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    return o


def _window(o, trace, w, layers):
    _, ev, labels = trace
    o.packed(ev, labels)
    o.window_close(w, layers)
    return o.edge_rows()


def test_adversarial_trace_reaches_the_edges(oracle_lib, trace):
    """the trace the GPU probes run on has what it promises: the row lengths of K4's slot and block boundaries, the table boundary
    of log1p_count, z beyond +-8, a source with sd <= 1 us, means below 100 ns, a max of 1e12 ns, open-connection-only rows and
    nodes, label and raw-IP outbound nodes"""
    o = _oracle(oracle_lib, trace)
    rows = _window(o, trace, np.zeros(pw.weights_count(1), np.float32), 1)
    deg = np.unique(rows["from_ref"], return_counts=True)[1]
    for d in pw.HUB_DEGREES:
        assert (deg == d).any(), d
    assert deg.max() > 1024
    assert {4095, 4096, 4097} <= set(rows["count"].tolist()) and {4095, 4096, 4097} <= set(rows["err_count"].tolist())
    e = pw.edge_features_ref(rows)
    assert (e[:, 6] == 1.0).any() and (e[:, 6] == -1.0).any()                 # clamped both ways
    m_ns = rows["sum_ns"] / np.maximum(rows["count"], 1)
    assert ((m_ns > 0) & (m_ns < 100)).any() and (m_ns == 100).any()
    assert ((m_ns > 50_000) & (m_ns < 100_000)).sum() >= 4 and (np.abs(m_ns - 414_213.56) < 20).sum() >= 2
    assert rows["max_ns"].max() == 1_000_000_000_000
    assert ((rows["count"] == 0) & (rows["alive"] > 0)).any()
    t = np.concatenate([rows["from_ref"], rows["to_ref"]]) >> 30
    assert (t == 1).any() and (t == 2).any()
    s, _ = o.node_stats()
    x = o.node_features()
    assert (x[:, 13] == 0).any() and ((s[:, 2] > 0) & (x[:, 13] > 0) & (x[:, 13] < np.log1p(1e-3))).any()   # sd <= 1 us with events
    assert (x[:, 16] > 0).any() and (x[:, 17] > 0).any()


@pytest.mark.parametrize("layers", [1, 2])
def test_oracle_readout_recovers_every_probed_quantity(oracle_lib, trace, layers):
    """every probe on the C oracle: the recovered phi equals what the oracle computed (node features, layer outputs) within half the
    readout bound, and the float64 restatement of the edge features within 1 fp32 ulp beyond it; the all-zero blob scores exactly
    0.5 and a blob of b2 alone scores sigmoid(b2) everywhere"""
    o = _oracle(oracle_lib, trace)
    worst = 0.0
    for p in pw.probes(layers):
        rows = _window(o, trace, p.w, layers)
        s = rows["score"]
        if p.kind == "const":
            b2 = float(p.w[-1])
            assert np.all(s == s[0]) and abs(float(s[0]) - 1.0 / (1.0 + np.exp(-b2))) < 1e-7, p.name
            if not p.w.any():
                assert np.all(s == np.float32(0.5))
            continue
        got = pw.readout(p, s)
        if p.kind == "edge":
            ref = pw.edge_features_ref(rows)[:, p.col]
            err = np.abs(got - pw.expected(p, ref))
            tol = pw.ulp32(ref) + p.bound() / 2
        else:
            phi = pw.oracle_phi(p, o, rows)
            err = np.abs(got - pw.expected(p, phi))
            tol = p.bound() / 2
            if p.kind in ("src", "dst"):
                assert np.array_equal(phi, o.node_features()[pw.dense_ids(o, rows)[0 if p.kind == "src" else 1], p.col])
        assert np.all(err <= tol), (p.name, float(err.max()), int(np.argmax(err - tol)))
        if p.kind != "edge":
            worst = max(worst, float((err * p.c).max()))
        assert np.ptp(got) > 0 or p.kind == "edge" and p.col == 7, p.name                # the probe reads something that varies
    # the measured readout error, in units of c * phi: inside half the derived bound (2^-21), with room to spare
    assert worst <= pw.READOUT_BOUND / 2, worst


def test_a_one_ulp_error_in_a_feature_shows_through_the_probe(oracle_lib, trace):
    """sensitivity: the readout resolves features to well under one fp32 ulp for phi >= 1 (at c = 8 the bound is 1.2e-7, an ulp of
    1 is 1.2e-7 and of 2 is 2.4e-7), where the score bar of 1e-5 would pass hundreds of ulps"""
    o = _oracle(oracle_lib, trace)
    p = next(q for q in pw.probes(1) if q.name == "src_x0")
    rows = _window(o, trace, p.w, 1)
    phi = pw.oracle_phi(p, o, rows)
    big = phi >= 2.0
    assert big.sum() > 100
    bumped = np.nextafter(phi[big], np.float32(np.inf))
    got = pw.readout(p, rows["score"])[big]
    assert np.all(np.abs(got - bumped) > p.bound())
