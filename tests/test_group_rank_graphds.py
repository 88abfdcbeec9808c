"""GraphDS's entries of the workload ranking (K17) against the recording stand-in engine of host_capi.cpp: SetWorkloadRank forwarded
with its parameters, WorkloadCulprits' rows named as WorkloadNodes names them, each with its rank row; and an engine library without
the entries (an older one)."""
import numpy as np

from alaz_amd import engine, hostlib

from tests.helpers import G


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


def test_the_switch_is_forwarded_with_its_parameters():
    ds = _ds()
    assert ds.set_workload_rank() == 0 and ds.set_workload_rank(iters=7, damping_q8=131, seed=engine.RANK_SEED["uniform"]) == 0
    assert ds.set_workload_rank(False) == 0
    assert [tuple(int(x) for x in r) for r in ds.mock_k17_ops()] == [(1, 0, 0, 0), (1, 7, 131, 1), (1,) + ((1 << 64) - 1,) * 3]


def test_culprits_are_named_and_carry_their_rank_rows():
    ds = _ds()
    assert ds.set_workload_rank() == 0
    rows, idx = ds.workload_culprits(5, 0.125)
    assert rows.dtype.itemsize == 16 + 160 + 136 + 16 and rows["node"]["row"].dtype == engine.NODE_DTYPE and rows["rank"].dtype == engine.RANK_DTYPE
    assert idx.tolist() == [1, 2]
    assert [(r["type"], r["uid"]) for r in rows["node"]] == [(b"workload", b"dep-a"), (b"pod", b"pod-0")]
    assert rows["node"]["row"]["ref"].tolist() == [G(0), 0] == rows["rank"]["ref"].tolist()
    assert rows["node"]["row"]["in_count"].tolist() == [9, 4] and rows["node"]["row"]["score"].tolist() == [0.5, 0.25]
    assert rows["rank"]["rank"].tolist() == [3 << 54, 1 << 53] and rows["rank"]["share"].tolist() == [0.75, 0.125]
    rows, idx = ds.workload_culprits(0)                               # k = 0: the count first, then the rows
    assert idx.tolist() == [1, 2] and len(rows) == 2 and rows["rank"]["share"][0] == 0.75
    rows, idx = ds.workload_culprits(1)                               # k below the selection: the first k
    assert idx.tolist() == [1] and rows["node"]["uid"][0] == b"dep-a"
    inf = _bits(float("-inf"))
    assert [tuple(int(x) for x in r) for r in ds.mock_k17_ops()] == \
        [(1, 0, 0, 0)] + [(2, 5, _bits(0.125), 5)] * 2 + [(2, 0, inf, 0), (2, 0, inf, 2)] * 2 + [(2, 1, inf, 1)] * 2


def test_the_rows_match_workload_nodes_naming():
    ds = _ds()
    nodes = ds.workload_nodes()
    rows, idx = ds.workload_culprits(2)
    for r, i in zip(rows, idx):
        assert (r["node"]["type"], r["node"]["uid"]) == (nodes["type"][i], nodes["uid"][i])
        assert r["node"]["row"]["ref"] == nodes["row"]["ref"][i]


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_workload_rank", "sgh_graphds_workload_culprits", "sgh_mock_k17_ops"):
        assert getattr(lib, name).argtypes is not None
