"""GraphDS's entries of the SLO burn rates (K24) against the recording stand-in engine of host_capi.cpp: SetSLO forwarded with its
spaces and parameters, SetWorkloadSLO resolving an owner UID to the workload's GROUP ref, WorkloadSLO's rows and WorkloadSLOTop's
rows named as WorkloadNodesTop names them."""
from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

ONES = (1 << 64) - 1
ERR_IN = engine.SLOSEL_BY["err"] | engine.SLOSEL_SIDE["in"]
GROUP_NODES = engine.Q_SPACES["group_nodes"]


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k24_ops()]


def test_the_switch_is_forwarded_with_its_spaces_and_parameters():
    ds = _ds()
    assert ds.set_slo() == 0                                          # the workload space, every default
    assert ds.set_slo(5, latency_bin=3, long_windows=64, min_requests=1 << 40) == 0
    assert ds.set_slo(0) == 0                                         # no space: off (the engine decides)
    assert ds.set_slo(4, on=False) == 0                               # no parameters: off
    assert ds.set_slo(2) == engine.SG_EINVAL                          # the engine's refusal comes back
    assert _ops(ds) == [(1, 4, 10 | 12 << 32, 100), (1, 5, 3 | 64 << 32, 1 << 40), (1, 0, 10 | 12 << 32, 100), (1, 4, ONES, 0), (1, 2, 10 | 12 << 32, 100)]


def test_a_workloads_objective_goes_to_its_group_ref():
    ds = _ds()
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")                  # node 1, workload 1 = sts-q
    word = engine.slo_objective(4, 999_000, 999_900)
    assert ds.set_workload_slo("sts-q", word) == 0 and ds.set_workload_slo("dep-a", 0) == 0
    assert ds.set_workload_slo("rs-a", word) == engine.SG_EINVAL      # a ReplicaSet is no workload: its Deployment is
    assert ds.set_workload_slo("nobody", word) == engine.SG_EINVAL and ds.set_workload_slo("", word) == engine.SG_EINVAL
    assert _ops(ds) == [(2, GROUP_NODES, engine.REF_GROUP << 30 | 1, word), (2, GROUP_NODES, engine.REF_GROUP << 30 | 0, 0)]


def test_the_rows_and_the_selection():
    ds = _ds()
    rows = ds.workload_slo()
    assert rows.shape == (3, engine.SLO_WORDS) and rows[2].tolist() == [200 + w for w in range(18)] and rows[0, 17] == 17
    top, idx = ds.workload_slo_top(ERR_IN, 5, 1024)
    assert idx.tolist() == [1, 2] and len(top) == 2
    plain, _ = ds.workload_nodes_top(engine.NSEL_BY["in_lat_dev"], 5, 0.5)
    assert top.dtype == plain.dtype
    assert top["row"]["ref"].tolist() == [(engine.REF_GROUP << 30) | 0, 0] and top["row"]["in_count"].tolist() == [9, 4]
    wn = ds.workload_nodes()                                          # the names are those of the rows at the selected indices
    assert top["type"].tolist() == wn["type"][idx].tolist() and top["uid"].tolist() == wn["uid"][idx].tolist()
    top0, idx0 = ds.workload_slo_top(engine.SLOSEL_BY["slow"] | engine.SLOSEL_SIDE["out"], 0)   # k = 0: the count first, then the rows
    assert idx0.tolist() == [1, 2]
    assert _ops(ds) == [(3, 0, 0, 0), (3, 3, 0, 0)] * 2 + [(4, ERR_IN, 5, 1024)] * 2 + [(4, 5, 0, 0)] * 4


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_slo", "sgh_graphds_set_workload_slo", "sgh_graphds_workload_slo", "sgh_graphds_workload_slo_top", "sgh_mock_k24_ops"):
        assert getattr(lib, name).argtypes is not None
