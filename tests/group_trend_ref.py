"""numpy reference of the workload baselines (K15, include/servicegraph.h "workload baselines"), of their vanished list and of the
selection over group edges.

A window's group edges (tests/group_ref.group_ref of its rows, or the device's own) are the samples, keyed by the workload keys of
their two group refs.  They run through tests/trend_ref.TrendRef's own update, as tests/node_trend_ref.py does it: its window
function is called with two of its module globals swapped for the group forms (the samples of a group edge, the keys of a group
edge), so the entry update, expiry, capacity cut and row rule are K8's code, not a copy.  GroupVanishRef does the same with
tests/vanish_ref.VanishRef's window function."""
import types

import numpy as np

from alaz_amd.engine import REF_GROUP, TREND_DTYPE
from tests import trend_ref, vanish_ref
from tests.node_trend_ref import x_err
from tests.select_by_ref import ref_select_by


def workload_keys(refs, obips):
    """wk of group refs: g for a group (key type 0), else (1 + type) << 32 | value, the IPv4 address (obips[value]) for OBIP refs"""
    r = np.asarray(refs, dtype=np.uint64)
    grp = (r >> np.uint64(30)) == REF_GROUP
    plain = np.where(grp, np.uint64(0), r)                            # (a group ref through ref_keys would read type 3 as a node type)
    return np.where(grp, r & np.uint64(0x3FFFFFFF), trend_ref.ref_keys(plain, obips) + np.uint64(1 << 32))


def group_keys(groups, obips):
    """trend_ref.row_keys for group edges: (wk(from_ref), wk(to_ref))"""
    return workload_keys(groups["from_ref"], obips), workload_keys(groups["to_ref"], obips)


def _samples(g):
    """trend_ref.samples for group edges (u64 counts): (live, x_lat, x_err)"""
    cnt = g["count"].astype(np.uint64)
    live = cnt > 0
    c = np.where(live, cnt, np.uint64(1))
    xl = np.minimum(g["sum_ns"].astype(np.uint64) // c, np.uint64(1 << 52)).astype(np.float64)
    return live, xl, x_err(g["err_count"], cnt)


_window = types.FunctionType(trend_ref.TrendRef.window.__code__, {**vars(trend_ref), "samples": _samples, "row_keys": group_keys},
                             "window")
_van_window = types.FunctionType(vanish_ref.VanishRef.window.__code__, {**vars(vanish_ref), "row_keys": group_keys}, "window")


class GroupTrendRef(trend_ref.TrendRef):
    """The workload baseline of one engine.  window(groups, obips) -> the window's TREND_DTYPE rows, row k for group edge k;
    .entries = the baseline afterwards."""

    def window(self, groups, obips):
        t = _window(self, groups, obips)
        assert t.dtype == TREND_DTYPE
        return t


class GroupVanishRef(vanish_ref.VanishRef):
    """window(groups, obips) -> (TREND_DTYPE rows, VANISHED_DTYPE list cut at max_rows, count of every vanished entry)"""

    def window(self, groups, obips):
        return _van_window(self, groups, obips)


def ref_select_groups(groups, gtrend, by, k, min_value):
    """group-edge positions K7 selects from `groups` by key `by` (a key of engine.SEL_BY), with gtrend the window's group trend rows
    (None for by = "score": score_max of the group edge)"""
    if by == "score":
        vals = np.zeros(len(groups), dtype=[("v", "<f4")])
        vals["v"] = groups["score_max"]
        return ref_select_by(None, vals, "v", k, min_value)
    return ref_select_by(groups, gtrend, by, k, min_value)
