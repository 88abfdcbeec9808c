"""GraphDS's entries of the traffic baselines (K23) against the recording stand-in engine of host_capi.cpp: SetTrafficTrend forwarded
with its spaces and parameters, and WorkloadTrafficTop's rows named as WorkloadNodesTop names them."""
import struct

from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

ONES = (1 << 64) - 1
DROP_IN = engine.TSEL_BY["drop"] | engine.TSEL_SIDE["in"]


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k23_ops()]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_the_switch_is_forwarded_with_its_spaces_and_parameters():
    ds = _ds()
    assert ds.set_traffic_trend() == 0                                # the node space, every default
    assert ds.set_traffic_trend(15, shift=3, warmup=2, ttl=9, rate_floor=5, load_floor_ns=7) == 0
    assert ds.set_traffic_trend(0) == 0                               # no space: off (the engine decides)
    assert ds.set_traffic_trend(8, on=False) == 0                     # no parameters: off
    assert ds.set_traffic_trend(16) == engine.SG_EINVAL               # the engine's refusal comes back
    assert _ops(ds) == [(1, 2, 0, 0), (1, 15, 3, 5 | 7 << 32), (1, 0, 0, 0), (1, 8, ONES, 0), (1, 16, 0, 0)]


def test_the_traffic_selection_names_its_rows_as_the_plain_one_does():
    ds = _ds()
    rows, idx = ds.workload_traffic_top(DROP_IN, 5, 0.5)
    assert idx.tolist() == [1, 2] and len(rows) == 2
    plain, _ = ds.workload_nodes_top(engine.NSEL_BY["in_lat_dev"], 5, 0.5)
    assert rows.dtype == plain.dtype
    assert rows["row"]["ref"].tolist() == [(engine.REF_GROUP << 30) | 0, 0] and rows["row"]["in_count"].tolist() == [9, 4]
    wn = ds.workload_nodes()                                          # the names are those of the rows at the selected indices
    assert rows["type"].tolist() == wn["type"][idx].tolist() and rows["uid"].tolist() == wn["uid"][idx].tolist()
    rows0, idx0 = ds.workload_traffic_top(engine.TSEL_BY["surge"] | engine.TSEL_SIDE["out"], 0)   # k = 0: the count first, then the rows
    assert idx0.tolist() == [1, 2]
    ninf = _bits(float("-inf"))
    assert _ops(ds) == [(2, DROP_IN, 5, _bits(0.5))] * 2 + [(2, 8, 0, ninf)] * 4


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_traffic_trend", "sgh_graphds_workload_traffic_top", "sgh_mock_k23_ops"):
        assert getattr(lib, name).argtypes is not None
