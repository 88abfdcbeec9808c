"""Pure-Python reference of the workload tracks (K19, include/servicegraph.h "workload tracks"): tests/track_ref.py's algorithm with
the workload anchor rule, as tests/group_nodes_ref.py swaps node_trend_ref's key function — TrackRef.step's own code runs with
is_anchor read as is_group_anchor.

GroupTrackRef(quiet_windows, max_tracks, ncap) is TrackRef over workload rows: step(workload rows, incident per workload row,
workload incident rows) -> (TRACK_DTYPE rows, the ended TRACK_ENTRY_DTYPE entries).  A row is an anchor when its ref is a GROUP,
KNOWN or LABEL ref (SG_REF_TYPE 3, 0 or 1); an OBIP ref (2) is an index into one window's outbound-IP list and anchors nothing.  The
members are keyed by ref — the device keys them by K16's group key, which is one-to-one with the ref below the outbound IPs — so a
pod moved to another group appears under another ref, and its old ref's member ages out.  ncap is the workload rows' capacity."""
import types

from tests.track_ref import TrackRef


def is_group_anchor(ref):
    return (int(ref) >> 30) in (0, 1, 3)


class GroupTrackRef(TrackRef):
    step = types.FunctionType(TrackRef.step.__code__, {**TrackRef.step.__globals__, "is_anchor": is_group_anchor}, "step")
