"""GraphDS's service binding (SetServiceBinding) against the recording stand-in engine of host_capi.cpp: the sg_group_assign calls
it makes (mock_group_ops).  A Service joins group g iff its Endpoints name at least one pod the store knows and every known pod
among them is in g; every event order ends in the same assignment; a rollout keeps it; two workloads behind one Service, a DELETE of
any of the objects and the switch going off take it back; with the switch never on the recorded calls are what they are without
the Service names and Endpoints; and an engine library without sg_group_assign refuses the switch."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from alaz_amd import engine, hostlib

from tests.host_scaffold import _ds

NO = engine.NO_GROUP
SET = 0xFFFFFFFE                                                      # mock_group_ops' marker of an sg_set_groups call


def _final(ds):
    """node id -> group after every recorded call, in order (an sg_set_groups call starts the map over)"""
    m = {}
    for node, group in ds.mock_group_ops().tolist():
        if node == SET:
            m = {}
        elif group == NO:
            m.pop(node, None)
        else:
            m[node] = group
    return m


EVENTS = {
    "svc": lambda ds: ds.PersistServiceNamed("svc-pay", "10.1.0.1", "payments", "shop"),
    "eps": lambda ds: ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-b"), ("Node", "n1"), ("Pod", "")]),
    "pod-a": lambda ds: ds.PersistPodOwned("pod-a", "10.0.0.1", "rs-1"),
    "pod-b": lambda ds: ds.PersistPodOwned("pod-b", "10.0.0.2", "rs-1"),
    "rs": lambda ds: ds.PersistReplicaSet("rs-1", "dep-pay"),
}


@pytest.mark.parametrize("when", ["first", "middle", "last"])
def test_every_event_order_ends_in_the_same_assignment(when):
    """the 120 orders of Service, Endpoints, two pods and their ReplicaSet, with the two switches in front, after two events or
    behind them all: the Service and both pods end in one group, and nothing else is assigned"""
    for order in itertools.permutations(EVENTS):
        ds = _ds()
        at = {"first": 0, "middle": 2, "last": len(order)}[when]
        for k, name in enumerate(order + (None,)):
            if k == at:
                assert ds.set_workload_groups(0) == 0 and ds.set_service_binding() == 0
            if name:
                assert EVENTS[name](ds) == 0
        m = _final(ds)
        assert len(m) == 3 and len(set(m.values())) == 1, (order, m)
        ops = ds.mock_group_ops().tolist()
        for (n0, g0), (n1, g1) in zip(ops, ops[1:]):                   # each change once: never the value the engine already holds
            assert (n0, g0) != (n1, g1)


def _bound():
    ds = _ds()
    assert ds.set_workload_groups(0) == 0 and ds.set_service_binding() == 0
    for name in ("rs", "pod-a", "pod-b", "svc", "eps"):
        EVENTS[name](ds)
    m = _final(ds)
    svc = [n for n in m if n not in (0, 1)]
    assert m == {0: 0, 1: 0, svc[0]: 0} and svc == [2]
    return ds


def test_a_rollout_keeps_the_assignment():
    """a second ReplicaSet of the same Deployment brings new pods, the Endpoints name old and new, then only the new: the Service
    stays in the Deployment's group and no call un-assigns it on the way"""
    ds = _bound()
    before = len(ds.mock_group_ops())
    ds.PersistReplicaSet("rs-2", "dep-pay")
    ds.PersistPodOwned("pod-c", "10.0.0.3", "rs-2")
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-b"), ("Pod", "pod-c")], "UPDATE")
    ds.PersistPodOwned("pod-a", "10.0.0.1", "rs-1", "DELETE"); ds.PersistPodOwned("pod-b", "10.0.0.2", "rs-1", "DELETE")
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-c")], "UPDATE")
    later = ds.mock_group_ops().tolist()[before:]
    assert later == [[3, 0]]                                          # pod-c joins; the Service (node 2) is never touched
    assert _final(ds)[2] == 0


def test_two_workloads_or_an_ungrouped_pod_behind_one_service_unassign_it():
    ds = _bound()
    ds.PersistPodOwned("pod-x", "10.0.0.9", "sts-other")              # another workload
    assert _final(ds)[2] == 0                                         # (not behind the Service yet)
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-x")], "UPDATE")
    assert 2 not in _final(ds) and ds.mock_group_ops().tolist()[-1] == [2, NO]
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a")], "UPDATE")
    assert _final(ds)[2] == 0
    ds.PersistPodOwned("pod-y", "10.0.0.10", "")                      # a pod without an owner is in no group
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-y")], "UPDATE")
    assert 2 not in _final(ds)
    ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-unknown")], "UPDATE")   # a pod the store does not know is not counted
    assert _final(ds)[2] == 0
    ds.PersistPodOwned("pod-a", "10.0.0.1", "sts-other", "UPDATE")    # re-owned: the Service follows its pod
    assert _final(ds)[2] == _final(ds)[0] == 1


@pytest.mark.parametrize("what", ["endpoints", "service", "pods", "empty"])
def test_delete_of_each_object(what):
    ds = _bound()
    if what == "endpoints":
        ds.PersistEndpoints("payments", "shop", [], "DELETE")
    elif what == "service":
        ds.PersistServiceNamed("svc-pay", "10.1.0.1", "payments", "shop", "DELETE")
    elif what == "pods":
        ds.PersistPodOwned("pod-a", "10.0.0.1", "rs-1", "DELETE")
        assert _final(ds)[2] == 0                                     # one known pod is left behind it
        ds.PersistPodOwned("pod-b", "10.0.0.2", "rs-1", "DELETE")
    else:
        ds.PersistEndpoints("payments", "shop", [], "UPDATE")         # Endpoints that name nobody
    assert 2 not in _final(ds) and ds.mock_group_ops().tolist()[-1] == [2, NO]
    n = len(ds.mock_group_ops())
    if what == "service":                                             # forgotten: its Endpoints no longer assign anything
        ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a")], "UPDATE")
        assert len(ds.mock_group_ops()) == n
    if what == "endpoints":                                           # and back
        EVENTS["eps"](ds)
        assert _final(ds)[2] == 0


def test_binding_off_afterwards_unassigns_and_on_again_assigns():
    ds = _bound()
    ds.PersistServiceNamed("svc-free", "10.1.0.2", "free", "shop")    # a Service without Endpoints: never assigned
    assert ds.set_service_binding(False) == 0
    assert ds.mock_group_ops().tolist()[-1] == [2, NO] and _final(ds) == {0: 0, 1: 0}
    n = len(ds.mock_group_ops())
    EVENTS["eps"](ds); EVENTS["svc"](ds)
    assert len(ds.mock_group_ops()) == n                              # off: the events assign nothing
    assert ds.set_service_binding(True) == 0
    assert _final(ds) == {0: 0, 1: 0, 2: 0}
    assert ds.set_workload_groups(0) == 0                             # the engine's map starts over: pods and the Service again
    assert _final(ds) == {0: 0, 1: 0, 2: 0}


def test_binding_never_on_leaves_the_ops_of_an_unbound_run_untouched():
    runs = []
    for named in (False, True):
        ds = _ds()
        assert ds.set_workload_groups(0) == 0
        ds.PersistReplicaSet("rs-1", "dep-pay")
        ds.PersistPodOwned("pod-a", "10.0.0.1", "rs-1")
        if named:
            ds.PersistServiceNamed("svc-pay", "10.1.0.1", "payments", "shop")
            ds.PersistEndpoints("payments", "shop", [("Pod", "pod-a"), ("Pod", "pod-b")])
        else:
            ds.PersistService("svc-pay", "10.1.0.1")
        ds.PersistPodOwned("pod-b", "10.0.0.2", "rs-1")
        ds.PersistPodOwned("pod-a", "10.0.0.1", "rs-1", "DELETE")
        ds.FlushWindow(1)
        if named:
            ds.PersistServiceNamed("svc-pay", "10.1.0.1", "payments", "shop", "DELETE")
            ds.PersistEndpoints("payments", "shop", [], "DELETE")
        else:
            ds.PersistService("svc-pay", "10.1.0.1", "DELETE")
        ds.FlushWindow(2)
        runs.append(ds.mock_group_ops().tolist())
    assert runs[0] == runs[1] and [SET, 0] in runs[0]


def test_the_switch_needs_the_workload_groups():
    ds = _ds()
    assert ds.set_service_binding() == engine.SG_ESTATE
    assert ds.set_workload_groups(0) == 0 and ds.set_service_binding() == 0


STUB = """
#include <stddef.h>
#include <stdint.h>
int sg_create(const void* c, void** h) { static int x; *h = &x; return 0; }
int sg_destroy(void* h) { return 0; }
int sg_upsert_pod(void* h, uint32_t ip, uint32_t id) { return 0; }
int sg_delete_pod(void* h, uint32_t ip) { return 0; }
int sg_upsert_service(void* h, uint32_t ip, uint32_t id) { return 0; }
int sg_delete_service(void* h, uint32_t ip) { return 0; }
int sg_set_label_count(void* h, uint32_t n) { return 0; }
int sg_ingest(void* h, const void* e, size_t n) { return 0; }
int sg_flush_window(void* h, uint64_t w, void* o, size_t c, size_t* n) { if (n) *n = 0; return 0; }
int sg_window_outbound_ips(void* h, uint32_t* o, size_t c, size_t* n) { if (n) *n = 0; return 0; }
const char* sg_last_error(void* h) { return ""; }
int sg_set_groups(void* h, const void* p) { return 0; }
"""


def test_an_engine_library_without_sg_group_assign(tmp_path):
    """an older engine: the required entries and sg_set_groups, no sg_group_assign — both switches are SG_EINVAL, events still pass"""
    src, lib = tmp_path / "old_engine.c", tmp_path / "libold_engine.so"
    src.write_text(STUB)
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(src)])
    ds = hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=str(lib))
    assert ds.set_workload_groups(0) == engine.SG_EINVAL and ds.set_service_binding() == engine.SG_EINVAL
    assert ds.set_workload_impact() == engine.SG_EINVAL
    for name in ("rs", "pod-a", "svc", "eps"):
        assert EVENTS[name](ds) == 0


def test_workload_impact_is_forwarded_and_paired_with_the_incidents():
    ds = _ds()
    assert ds.set_workload_impact() == 0 and ds.set_workload_impact(64, 3) == 0 and ds.set_workload_impact(0, 0) == 0
    inc, rows = ds.workload_impact()
    # (the binding asks twice, for the sizes and for the rows; GraphDS reads the count, then the rows, each time)
    assert ds.mock_k22_ops().tolist() == [[1, 256, 8, 0], [1, 64, 3, 0], [1, 0, 0, 0]] + [[2, 0, 0, 0], [2, 2, 0, 0]] * 2
    assert len(inc) == 2 and rows.shape == (2, engine.IMPACT_WORDS) and rows.dtype == np.uint64
    assert inc["first_node"].tolist() == [0, 1] and inc["nodes"].tolist() == [2, 1]
    assert rows.tolist() == [[1, 1, 1 << 32 | 1, 1, 40, 3, 7, 2], [0, 0, 0xFFFFFFFF, 1, 4, 0, 0, 0]]


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_persist_service_named", "sgh_graphds_persist_endpoints", "sgh_graphds_set_service_binding",
                 "sgh_graphds_set_workload_impact", "sgh_graphds_workload_impact", "sgh_mock_k22_ops"):
        assert getattr(lib, name).argtypes is not None
