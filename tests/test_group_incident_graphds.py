"""GraphDS's entries of the workload incidents (K18) against the recording stand-in engine of host_capi.cpp: SetWorkloadIncidents
forwarded with its parameters, WorkloadIncidents' rows and the incident per workload row as the engine gives them."""
import numpy as np

from alaz_amd import engine, hostlib

ONES = (1 << 64) - 1


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _ds():
    ds = hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")                  # node 1, workload 1 = sts-q
    assert ds.set_workload_nodes() == 0
    return ds


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k18_ops()]


def test_the_switch_is_forwarded_with_its_parameters():
    ds = _ds()
    assert ds.set_workload_incidents(min_value=0.5) == 0
    assert ds.set_workload_incidents(by=engine.SEL_BY["lat_dev"], min_value=3.0) == 0
    assert ds.set_workload_incidents(False) == 0
    assert _ops(ds) == [(1, 0, _bits(0.5), 0), (1, 1, _bits(3.0), 0), (1, ONES, ONES, ONES)]


def test_incident_rows_and_the_incident_per_workload_row():
    ds = _ds()
    assert ds.set_workload_incidents(min_value=0.5) == 0
    rows, inc = ds.workload_incidents()
    assert rows.dtype == engine.INCIDENT_DTYPE and inc.dtype == np.uint32
    assert inc.tolist() == [0, 1, 0]
    assert rows["first_node"].tolist() == [0, 1] and rows["nodes"].tolist() == [2, 1] and rows["edges"].tolist() == [2, 1]
    assert rows["count"].tolist() == [9, 4] and rows["err"].tolist() == [2, 0] and rows["sum_ns"].tolist() == [900, 0]
    assert rows["worst_row"].tolist() == [1, 2] and rows["value_max"].tolist() == [0.75, 0.5]
    assert rows["top_node"].tolist() == [2, 1] and rows["culprit_node"].tolist() == [2, engine.NO_INCIDENT]
    assert rows["rank_sum"].tolist() == [3 << 54, 0] and rows["reserved"].tolist() == [0, 0]
    # the count first, then the rows; the same for the incident per row
    assert _ops(ds) == [(1, 0, _bits(0.5), 0)] + [(2, 0, 0, 0), (2, 2, 0, 0), (3, 0, 0, 0), (3, 0, 3, 0)] * 2
    nodes = ds.workload_nodes()
    assert len(nodes) == len(inc)                                      # one incident number per row of workload_nodes()


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_workload_incidents", "sgh_graphds_workload_incidents", "sgh_mock_k18_ops"):
        assert getattr(lib, name).argtypes is not None
