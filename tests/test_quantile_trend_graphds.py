"""GraphDS's entries of the tail baselines (K21) against the recording stand-in engine of host_capi.cpp: SetTailTrend forwarded
with its spaces, per-mille and parameters, the three tail reads' rows as the engine gives them, and WorkloadTailTop's rows named
as WorkloadNodesTop names them."""
import struct


from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

ONES = (1 << 64) - 1


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k21_ops()]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_the_switch_is_forwarded_with_its_spaces_per_mille_and_parameters():
    ds = _ds()
    assert ds.set_tail_trend() == 0                                   # the node space, p99, every default
    assert ds.set_tail_trend(7, 999, shift=3, warmup=2, ttl=9) == 0
    assert ds.set_tail_trend(0) == 0                                  # no space: off (the engine decides)
    assert ds.set_tail_trend(2, 500, on=False) == 0                   # no parameters: off
    assert ds.set_tail_trend(8) == engine.SG_EINVAL                   # the engine's refusal comes back
    assert _ops(ds) == [(1, 1, 990, 0), (1, 7, 999, 3), (1, 0, 990, 0), (1, 2, 500, ONES), (1, 8, 990, 0)]


def test_tail_rows_come_out_as_the_engine_gives_them():
    ds = _ds()
    n, e, w = ds.node_tail_trends(), ds.workload_edge_tail_trends(), ds.workload_tail_trends()
    assert n.dtype == w.dtype == engine.NODE_TREND_DTYPE and e.dtype == engine.TREND_DTYPE
    assert n["in_seen"].tolist() == [20, 21, 22] and n["in_lat_dev"].tolist() == [10.0] * 3
    assert e["windows_seen"].tolist() == [30, 31, 32] and e["lat_dev"].tolist() == [11.0] * 3
    assert w["in_seen"].tolist() == [40, 41, 42] and w["in_lat_dev"].tolist() == [12.0] * 3
    # the count first, then the rows; the wrapper asks twice, for the size and for the rows
    assert _ops(ds) == [(2, 0, 0, 0), (2, 3, 0, 0)] * 2 + [(3, 0, 0, 0), (3, 3, 0, 0)] * 2 + [(4, 0, 0, 0), (4, 3, 0, 0)] * 2


def test_the_tail_selection_names_its_rows_as_the_plain_one_does():
    ds = _ds()
    rows, idx = ds.workload_tail_top(engine.NSEL_BY["in_lat_dev"], 5, 0.5)
    assert idx.tolist() == [1, 2] and len(rows) == 2
    plain, _ = ds.workload_nodes_top(engine.NSEL_BY["in_lat_dev"], 5, 0.5)
    assert rows.dtype == plain.dtype
    assert rows["row"]["ref"].tolist() == [(engine.REF_GROUP << 30) | 0, 0] and rows["row"]["in_count"].tolist() == [9, 4]
    wn = ds.workload_nodes()                                          # the names are those of the rows at the selected indices
    assert rows["type"].tolist() == wn["type"][idx].tolist() and rows["uid"].tolist() == wn["uid"][idx].tolist()
    rows0, idx0 = ds.workload_tail_top(engine.NSEL_BY["new"], 0)      # k = 0: the count first, then the rows
    assert idx0.tolist() == [1, 2]
    ninf = _bits(float("-inf"))
    assert _ops(ds) == [(5, 1, 5, _bits(0.5))] * 2 + [(5, 5, 0, ninf)] * 4


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_tail_trend", "sgh_graphds_tail_trends", "sgh_graphds_workload_tail_top", "sgh_mock_k21_ops"):
        assert getattr(lib, name).argtypes is not None
