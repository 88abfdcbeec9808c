"""GraphDS's entries of the workload tracks (K19) against the recording stand-in engine of host_capi.cpp: SetWorkloadTracks forwarded
with its parameters, WorkloadIncidentTracks' rows and WorkloadTracksEnded's list as the engine gives them."""
from alaz_amd import engine, hostlib

ONES = (1 << 64) - 1


def _ds():
    ds = hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)
    assert ds.set_workload_groups(0) == 0
    ds.PersistReplicaSet("rs-a", "dep-a")
    ds.PersistPodOwned("pod-0", "10.0.0.1", "rs-a")                   # node 0, workload 0 = dep-a
    ds.PersistPodOwned("pod-1", "10.0.0.2", "sts-q")                  # node 1, workload 1 = sts-q
    assert ds.set_workload_nodes() == 0 and ds.set_workload_incidents(min_value=0.5) == 0
    return ds


def _ops(ds):
    return [tuple(int(x) for x in r) for r in ds.mock_k19_ops()]


def test_the_switch_is_forwarded_with_its_parameters():
    ds = _ds()
    assert ds.set_workload_tracks() == 0
    assert ds.set_workload_tracks(quiet_windows=0, max_tracks=12) == 0
    assert ds.set_workload_tracks(False) == 0
    assert _ops(ds) == [(1, 2, 0, 0), (1, 0, 12, 0), (1, ONES, ONES, ONES)]


def test_rows_and_the_ended_list_come_out_as_the_engine_gives_them():
    ds = _ds()
    assert ds.set_workload_tracks(quiet_windows=1) == 0
    rows, ended = ds.workload_incident_tracks(), ds.workload_tracks_ended()
    assert rows.dtype == engine.TRACK_DTYPE and ended.dtype == engine.TRACK_ENTRY_DTYPE
    assert len(rows) == len(ds.workload_incidents()[0])                # one track row per incident row
    assert rows.tolist() == [(4, engine.NO_TRACK, 1, 3, 2, 0, 0, 0), (7, 4, 3, 1, 0, 0, 1, engine.TRACK_NEW | engine.TRACK_SPLIT)]
    assert ended.tolist() == [(5, 4, 1, 2, 2, 3, 17, 2)]
    # the count first, then the rows; the wrapper asks twice, for the size and for the rows
    assert _ops(ds) == [(1, 1, 0, 0)] + [(2, 0, 0, 0), (2, 2, 0, 0)] * 2 + [(3, 0, 0, 0), (3, 1, 0, 0)] * 2


def test_hostlib_declares_the_entries():
    lib = hostlib.load()
    for name in ("sgh_graphds_set_workload_tracks", "sgh_graphds_workload_incident_tracks", "sgh_graphds_workload_tracks_ended",
                 "sgh_mock_k19_ops"):
        assert getattr(lib, name).argtypes is not None
