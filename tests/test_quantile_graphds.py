"""GraphDS's entries of the latency percentiles (K20) against the recording stand-in engine of host_capi.cpp: SetQuantiles forwarded
with its spaces and per-mille, NodeLatency / WorkloadEdgeLatency / WorkloadLatency's rows as the engine gives them."""
import numpy as np

from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

ONES = (1 << 64) - 1


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k20_ops()]


def test_the_switch_is_forwarded_with_its_spaces_and_per_mille():
    ds = _ds()
    assert ds.set_quantiles() == 0
    assert ds.set_quantiles(7, (1, 1000, 999)) == 0
    assert ds.set_quantiles(2, ()) == 0                               # no per-mille: the engine's default
    assert ds.set_quantiles(0) == 0
    assert ds.set_quantiles(1, tuple(range(1, 10))) == engine.SG_EINVAL    # the engine's refusal comes back
    assert _ops(ds) == [(1, 1, 2, 500 | 990 << 16), (1, 7, 3, 1 | 1000 << 16 | 999 << 32), (1, 2, 0, 0), (1, 0, 2, 500 | 990 << 16),
                        (1, 1, 9, 1 | 2 << 16 | 3 << 32 | 4 << 48)]


def test_rows_come_out_as_the_engine_gives_them_in_the_shape_of_n_q():
    ds = _ds()
    assert ds.set_quantiles(7, (500, 990, 999)) == 0
    n, e, w = ds.node_latency(), ds.workload_edge_latency(), ds.workload_latency()
    assert n.dtype == e.dtype == w.dtype == np.uint32
    assert n.shape == (3, 2, 3) and e.shape == (3, 3) and w.shape == (3, 2, 3)
    assert n.reshape(-1).tolist() == list(range(20, 38)) and e.reshape(-1).tolist() == list(range(30, 39)) and w[0, 0].tolist() == [40, 41, 42]
    i = ds.workload_latency([2, 0])                                   # an index: those rows only
    assert i.shape == (2, 2, 3) and i.reshape(-1).tolist() == list(range(40, 52))
    assert ds.node_latency([]).shape == (0, 2, 0)
    # without an index the count first, then the rows; the wrapper asks twice, for the size and for the rows
    assert _ops(ds) == [(1, 7, 3, 500 | 990 << 16 | 999 << 32)] + [(2, ONES, 0, 0), (2, ONES, 3, 0)] * 2 + [(3, ONES, 0, 0), (3, ONES, 3, 0)] * 2 \
        + [(4, ONES, 0, 0), (4, ONES, 3, 0)] * 2 + [(4, 2, 2, 0)] * 2 + [(2, 0, 0, 0)] * 0
    assert ds.set_quantiles(1, ()) == 0
    assert ds.node_latency().shape == (3, 2, 2)                       # n_q = 0: {500, 990}


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_quantiles", "sgh_graphds_latency", "sgh_mock_k20_ops"):
        assert getattr(lib, name).argtypes is not None
