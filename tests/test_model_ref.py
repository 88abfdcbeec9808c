"""The plain references of tests/model_ref.py against the C oracle: node statistics word for word, node features within 1 fp32 ulp,
every SAGE layer within the derived forward-error bound; on the adversarial trace and on the boundary trace, whose promised shapes
are checked here on the oracle's rows.  No GPU."""
import numpy as np
import pytest

from tests.helpers import CLOCK
from tests import model_ref as mr
from tests import probe_weights as pw

TRACES = {"adversarial": pw.adversarial_trace, "boundary": mr.boundary_trace}


def closed(oracle_lib, name, layers):
    """the oracle's window of trace `name` under make_weights(layers) (model_ref.oracle_window: closed once)"""
    return mr.oracle_window(name, TRACES[name], layers, CLOCK)


@pytest.mark.parametrize("name", list(TRACES))
def test_oracle_node_stats_equal_a_recount_from_its_rows(oracle_lib, name):
    """Oracle.node_stats(): twelve sum words and two maxima per node, each equal to a recount from edge_rows()"""
    c = closed(oracle_lib, name, 1)
    s, m = c["stats"]
    assert s.shape == (c["n"], 12) and m.shape == (c["n"], 2) and s.dtype == np.uint64
    rs, rm = mr.node_stats_ref(c["rows"], c["n"], c["u"], c["v"])
    assert np.array_equal(s, rs) and np.array_equal(m, rm)
    rows, u, v = c["rows"], c["u"], c["v"]
    assert np.array_equal(s[:, mr.ST_OUT_DEG], np.bincount(u, minlength=c["n"])) and np.array_equal(s[:, mr.ST_IN_DEG], np.bincount(v, minlength=c["n"]))
    assert np.array_equal(s[:, mr.ST_OUT_CNT], np.bincount(u, weights=rows["count"], minlength=c["n"]).astype(np.uint64))
    assert np.array_equal(s[:, mr.ST_IN_CNT], np.bincount(v, weights=rows["count"], minlength=c["n"]).astype(np.uint64))
    assert s[:, mr.ST_OUT_ALIVE].sum() == rows["alive"].sum() > 0


@pytest.mark.parametrize("name", list(TRACES))
def test_oracle_node_features_within_one_ulp_of_the_float64_reference(oracle_lib, name):
    c = closed(oracle_lib, name, 1)
    ref = mr.node_features_ref(c["stats"], c["kind"])
    d = mr.ulp_distance(c["x0"], ref)
    print(f"{name}: {int((d != 0).sum())} of {d.size} elements of x0 are not bit-equal to the float64 reference (max {int(d.max())} ulp)")
    assert d.max() <= 1, (int(d.max()), np.argwhere(d > 1)[:4])
    assert np.all(c["x0"][:, 18:] == 0) and np.all(c["x0"][:, 15] == 1)
    assert np.array_equal(c["x0"][:, 10:13], ref[:, 10:13]) and np.all(c["x0"][:, 10:13].sum(axis=1) == 1)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("name", list(TRACES))
def test_oracle_layers_within_the_derived_bound_of_the_float64_layer(oracle_lib, name, layers):
    """layer_output(l) against sage_layer_ref of the oracle's own layer_output(l - 1) / x0: every element within its bound"""
    c = closed(oracle_lib, name, layers)
    rowptr, col = mr.csr_of(c["u"], c["v"], c["n"])
    for l in range(layers):
        hin = c["x0"] if l == 0 else c["h"][l]
        ref, bound = mr.sage_layer_ref(hin, rowptr, col, *mr.layer_weights(c["w"], l))
        err = np.abs(c["h"][l + 1].astype(np.float64) - ref)
        print(f"{name} L={layers} layer {l}: max error {err.max():.3e}, smallest room {np.min(bound - err):.3e}, max error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), (l, np.argwhere(err > bound)[:4])
        assert (np.ptp(ref[:, 1:], axis=0) > 0).sum() >= 32                  # dense weights: most of the units 1..63 are alive and vary


def test_boundary_trace_reaches_the_edges(oracle_lib):
    """what boundary_trace promises, on the oracle's rows: three node ranges; in-edges at 3071, 3072, 6143, 6144 and N - 1 from rows
    in different slices at every slice count the GPU tests use; an in-only and an out-only node next to a boundary; a destination with
    more than 1024 sources all over the CSR; one out-row of every length in BOUNDARY_DEGREES; several 8192-edge trips; and on every row
    of more than 16 neighbours the pinned-order fp32 mean of x0 differs from the left-to-right one"""
    c = closed(oracle_lib, "boundary", 1)
    n, rows, u, v = c["n"], c["rows"], c["u"], c["v"]
    E = len(rows)
    s, _ = c["stats"]
    assert 2 * mr.K3_RANGE < n <= 3 * mr.K3_RANGE
    assert 2 * 8192 < E < 32768
    t = np.concatenate([rows["from_ref"], rows["to_ref"]]) >> 30
    assert (t == 1).any() and (t == 2).any()
    assert s[mr.IN_ONLY, mr.ST_OUT_DEG] == 0 and s[mr.IN_ONLY, mr.ST_IN_DEG] >= 4
    assert s[mr.OUT_ONLY, mr.ST_IN_DEG] == 0 and s[mr.OUT_ONLY, mr.ST_OUT_DEG] >= 2
    for b in mr.BOUNDARY_NODES + (n - 1,):
        pos = np.flatnonzero(v == b)
        assert len(pos) >= 4, b
        for S in (2, 5, 8, 33, 47, 48):                                       # k3_in_part: slice = position // ceil(E / S)
            assert len(np.unique(pos // -(-E // S))) >= 2, (b, S)
    assert rows["count"][v == n - 1].sum() > 0
    pos = np.flatnonzero(v == mr.MANY_IN)
    assert len(pos) > 1024
    for S in (2, 5, 8, 33, 47, 48):
        assert len(np.unique(pos // -(-E // S))) >= min(S, 4), S
    deg = np.bincount(u, minlength=n)
    for d in mr.BOUNDARY_DEGREES:
        assert (deg[mr.BOUNDARY_PODS - len(mr.BOUNDARY_DEGREES):mr.BOUNDARY_PODS] == d).sum() == 1, d
    assert (deg == 0).any() and -(-deg.max() // mr.MEAN_BLOCK) == 10
    assert (s[:, mr.ST_OUT_ALIVE] > 0).any() and ((rows["count"] == 0) & (rows["alive"] > 0)).any()
    rowptr, col = mr.csr_of(u, v, n)
    for r in np.flatnonzero(deg > 16):
        nbr = col[rowptr[r]:rowptr[r + 1]]
        assert not np.array_equal(mr.pinned_mean32(c["x0"], nbr), mr.plain_mean32(c["x0"], nbr)), (int(r), int(deg[r]))
