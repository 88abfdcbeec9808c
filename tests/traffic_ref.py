"""numpy references of the traffic baselines (K23, include/servicegraph.h "traffic baselines"): one per space, and of the selections
by a traffic row.

Each is the mean baseline's reference of its space with BOTH samples swapped: tests/trend_ref.TrendRef.window's own code runs with
`samples` replaced by the traffic form — x_rate = 1000.0 * min(count, 2^42) in the latency half, x_load = min(sum_ns, 2^52) in the
error half — and with `row_keys` the key function of tests/trend_ref.py, tests/node_trend_ref.py, tests/group_trend_ref.py or the
workload form of tests/group_nodes_ref.py.  The entry update, expiry, capacity cut and row rule are K8's code, not a copy.  The
floors reach the walk as lat_floor = 1000.0 * rate_floor and err_floor = load_floor_ns."""
import types

import numpy as np

from alaz_amd.engine import NODE_TREND_DTYPE, TREND_DTYPE, TSEL_BY, TSEL_SIDE
from tests import group_nodes_ref, group_trend_ref, node_trend_ref, trend_ref
from tests.select_by_ref import ref_select_by

RATE_CLAMP, LOAD_CLAMP = 1 << 42, 1 << 52
RATE_FLOOR, LOAD_FLOOR_NS = 8, 1_000_000                             # the defaults of sg_traffic_params


def traffic_samples(s):
    """trend_ref.samples for traffic: (live, x_rate, x_load) of samples with `count` and `sum_ns` (edge rows, group edges, the
    node samples of node_trend_ref.node_samples)"""
    cnt = s["count"].astype(np.uint64)
    xr = 1000.0 * np.minimum(cnt, np.uint64(RATE_CLAMP)).astype(np.float64)
    xl = np.minimum(s["sum_ns"].astype(np.uint64), np.uint64(LOAD_CLAMP)).astype(np.float64)
    return cnt > 0, xr, xl


def _window_with(row_keys):
    return types.FunctionType(trend_ref.TrendRef.window.__code__, {**vars(trend_ref), "samples": traffic_samples, "row_keys": row_keys}, "window")


_edge_window = _window_with(trend_ref.row_keys)
_node_window = _window_with(node_trend_ref._keys)
_group_window = _window_with(group_trend_ref.group_keys)
_workload_window = _window_with(group_nodes_ref._keys)


def floors(rate_floor=0, load_floor_ns=0):
    """(lat_floor_ns, err_floor) as TrendRef takes them, a 0 resolved to its default"""
    return 1000 * (rate_floor or RATE_FLOOR), load_floor_ns or LOAD_FLOOR_NS


def _fold_sides(t, n):
    assert t.dtype == TREND_DTYPE
    out = np.zeros(n, dtype=NODE_TREND_DTYPE)
    for side, k in (("in", 0), ("out", 1)):
        h = t[k::2]
        out[f"{side}_lat_dev"], out[f"{side}_err_dev"] = h["lat_dev"], h["err_dev"]
        out[f"{side}_base_mean_us"], out[f"{side}_seen"] = h["base_mean_us"], h["windows_seen"]
    return out


class EdgeTrafficRef(trend_ref.TrendRef):
    """SG_T_EDGES (max_edges: the capacity default is K8's 2 x max_edges).  window(rows, obips) -> TREND_DTYPE rows"""

    def __init__(self, max_edges, shift=4, warmup=4, ttl=64, max_entries=0, rate_floor=0, load_floor_ns=0):
        super().__init__(max_edges, shift, warmup, ttl, max_entries, *floors(rate_floor, load_floor_ns))

    def window(self, rows, obips):
        t = _edge_window(self, rows, obips)
        assert t.dtype == TREND_DTYPE
        return t


class GroupTrafficRef(EdgeTrafficRef):
    """SG_T_GROUPS (K15's capacity default, 2 x max_edges).  window(groups, obips) -> TREND_DTYPE rows"""

    def window(self, groups, obips):
        t = _group_window(self, groups, obips)
        assert t.dtype == TREND_DTYPE
        return t


class NodeTrafficRef(node_trend_ref.NodeTrendRef):
    """SG_T_NODES (ncap: the capacity default is K10's 4 x ncap).  window(nodes, obips) -> NODE_TREND_DTYPE rows"""

    def __init__(self, ncap, shift=4, warmup=4, ttl=64, max_entries=0, rate_floor=0, load_floor_ns=0):
        super().__init__(ncap, shift, warmup, ttl, max_entries, *floors(rate_floor, load_floor_ns))

    def window(self, nodes, obips):
        return _fold_sides(_node_window(self, node_trend_ref.node_samples(nodes), obips), len(nodes))


class WorkloadTrafficRef(NodeTrafficRef):
    """SG_T_GROUP_NODES (nc: the row capacity).  window(workload rows, obips) -> NODE_TREND_DTYPE rows (K16's keys)"""

    def window(self, nodes, obips):
        return _fold_sides(_workload_window(self, node_trend_ref.node_samples(nodes), obips), len(nodes))


def traffic_column(traffic, by, side=None):
    """the SIGNED value a traffic key ranks: by a direction of TSEL_BY, side "in" / "out" for NODE_TREND_DTYPE rows, None for
    TREND_DTYPE rows.  The sign flips as the device flips it: the sign bit alone, so a NaN stays a NaN and +0.0 becomes -0.0"""
    assert by in TSEL_BY and (side is None or side in TSEL_SIDE)
    half = "lat_dev" if by in ("surge", "drop") else "err_dev"
    v = np.ascontiguousarray(traffic[half if side is None else f"{side}_{half}"], dtype=np.float32)
    if by in ("drop", "load_down"):
        v = (v.view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)
    return v


def ref_select_traffic(traffic, by, side, k, min_value):
    """row positions K7 selects by a traffic key: the rule of ref_select_nodes / ref_select_groups (tests/select_by_ref.py: value >=
    min_value, NaN never, k = 0 every candidate in row order, else the k highest descending, ties — -0.0 == +0.0 — by row
    position) over the signed column"""
    vals = np.zeros(len(traffic), dtype=[("v", "<f4")])
    vals["v"] = traffic_column(traffic, by, side)
    return ref_select_by(None, vals, "v", k, min_value)
