"""GraphDS's entries of the replica outliers (K25) against the recording stand-in engine of host_capi.cpp: SetReplicaOutliers forwarded
with its parameters (sg_set_replicas), WorkloadReplicaOutliers' selection named by pod UID and workload owner UID, with the words of
the side `by` names."""
from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

ONES = (1 << 64) - 1
ERR_IN = engine.RSEL_BY["err"] | engine.RSEL_SIDE["in"]
LAT_OUT = engine.RSEL_BY["lat"] | engine.RSEL_SIDE["out"]


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k25_ops()]


def test_the_switch_is_forwarded_with_its_parameters():
    ds = _ds()
    assert ds.set_replica_outliers() == 0                             # every default: zeros go through, the engine fills them in
    assert ds.set_replica_outliers(min_replicas=5, min_requests=1 << 40, min_err_excess_q20=7, min_lat_ratio_q10=9, tail_permille=990) == 0
    assert ds.set_replica_outliers(on=False) == 0                     # no parameters: off
    assert ds.set_replica_outliers(min_replicas=1) == engine.SG_EINVAL   # the engine's refusal comes back
    assert _ops(ds) == [(1, 0, 0, 0), (1, 5 | 990 << 32, 1 << 40, 7 | 9 << 32), (1, ONES, 0, 0), (1, 1, 0, 0)]


def test_the_selection_is_named_by_pod_and_workload():
    ds = _ds()
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "rs-a")                   # node 1
    top = ds.workload_replica_outliers(ERR_IN, 5, 1)
    assert top["pod"].tolist() == [b"pod-1", b"pod-0"] and top["workload"].tolist() == [b"dep-a"] * 2   # workload row 1 is GROUP 0
    assert top["node_index"].tolist() == [2, 0] and top["workload_index"].tolist() == [1, 1] and top["flags"].tolist() == [201, 1]
    assert top["err_excess_q20"].tolist() == [202, 2] and top["lat_ratio_q10"].tolist() == [203, 3] and top["share_q10"].tolist() == [204, 4]
    assert top["tail_pod"].tolist() == [205, 5] and top["tail_peers"].tolist() == [0, 0] and top["replicas"].tolist() == [206, 6]
    out = ds.workload_replica_outliers(LAT_OUT, 0)                    # k = 0: the count first, then the rows; the out side's words
    assert out["err_excess_q20"].tolist() == [207, 7] and out["replicas"].tolist() == [211, 11]
    assert _ops(ds) == [(3, ERR_IN, 5, 1), (2, 2, 2, 0)] * 2 + [(3, LAT_OUT, 0, 0), (3, LAT_OUT, 0, 0), (2, 2, 2, 0)] * 2


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_replica_outliers", "sgh_graphds_workload_replica_outliers", "sgh_mock_k25_ops"):
        assert getattr(lib, name).argtypes is not None
