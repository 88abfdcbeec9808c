"""numpy references of the tail baselines (K21, include/servicegraph.h "tail baselines"): one per K20 space.

Each is the mean baseline's reference of its space with the latency sample swapped: tests/trend_ref.TrendRef.window's own code runs
with `samples` replaced by a form whose x_lat = 1000.0 * Q — Q the tracked quantile of the entity and side, from
tests/quantile_ref.py on the same window (or the engine's own quantile read) — and with `row_keys` the key function of
tests/node_trend_ref.py, tests/group_trend_ref.py or the workload form of tests/group_nodes_ref.py.  The counts and the error
sample are those of the mean baseline, so the entry update, expiry, capacity cut and row rule are K8's code, not a copy.

Side order: quantile tables hold a node's sides as [0] = out, [1] = in; the samples are side 0 = in, 1 = out: sample 2k + s reads
q[k][1 - s]."""
import types

import numpy as np

from alaz_amd.engine import NODE_TREND_DTYPE, TREND_DTYPE
from tests import group_nodes_ref, group_trend_ref, node_trend_ref, trend_ref
from tests.node_trend_ref import x_err

#: a node sample and its tracked quantile; a group edge as a sample
NODE_SAMPLE_DTYPE = np.dtype(node_trend_ref.SAMPLE_DTYPE.descr + [("q", "<u4")])
GROUP_SAMPLE_DTYPE = np.dtype([("from_ref", "<u4"), ("to_ref", "<u4"), ("count", "<u8"), ("err_count", "<u8"), ("q", "<u4")])


def node_tail_samples(nodes, q):
    """the 2N samples of a window's node rows (or workload rows) with q [N][2] (out, in) the tracked quantile in microseconds"""
    base = node_trend_ref.node_samples(nodes)
    s = np.zeros(len(base), dtype=NODE_SAMPLE_DTYPE)
    for f in base.dtype.names:
        s[f] = base[f]
    q = np.asarray(q, dtype=np.uint32).reshape(len(nodes), 2)
    s["q"][0::2] = q[:, 1]                                            # side 0 = in  <- table side 1
    s["q"][1::2] = q[:, 0]                                            # side 1 = out <- table side 0
    return s


def group_tail_samples(groups, q):
    s = np.zeros(len(groups), dtype=GROUP_SAMPLE_DTYPE)
    for f in ("from_ref", "to_ref", "count", "err_count"):
        s[f] = groups[f]
    s["q"] = np.asarray(q, dtype=np.uint32).reshape(len(groups))
    return s


def _tail_samples(err_field):
    def samples(s):
        """trend_ref.samples for tail samples: (live, 1000.0 * Q, the mean baseline's x_err)"""
        cnt = s["count"].astype(np.uint64)
        return cnt > 0, 1000.0 * s["q"].astype(np.float64), x_err(s[err_field], cnt)
    return samples


def _window_with(samples, row_keys):
    return types.FunctionType(trend_ref.TrendRef.window.__code__, {**vars(trend_ref), "samples": samples, "row_keys": row_keys}, "window")


_node_window = _window_with(_tail_samples("err"), node_trend_ref._keys)
_group_window = _window_with(_tail_samples("err_count"), group_trend_ref.group_keys)
_workload_window = _window_with(_tail_samples("err"), group_nodes_ref._keys)


def _fold_sides(t, n):
    assert t.dtype == TREND_DTYPE
    out = np.zeros(n, dtype=NODE_TREND_DTYPE)
    for side, k in (("in", 0), ("out", 1)):
        h = t[k::2]
        out[f"{side}_lat_dev"], out[f"{side}_err_dev"] = h["lat_dev"], h["err_dev"]
        out[f"{side}_base_mean_us"], out[f"{side}_seen"] = h["base_mean_us"], h["windows_seen"]
    return out


class NodeTailRef(node_trend_ref.NodeTrendRef):
    """SG_Q_NODES.  window(nodes, q [N][2], obips) -> NODE_TREND_DTYPE rows; .entries = the baseline (K10's keys)."""

    def window(self, nodes, q, obips):
        return _fold_sides(_node_window(self, node_tail_samples(nodes, q), obips), len(nodes))


class GroupTailRef(trend_ref.TrendRef):
    """SG_Q_GROUPS (max_edges: the capacity default is K15's 2 x max_edges).  window(groups, q [G], obips) -> TREND_DTYPE rows"""

    def window(self, groups, q, obips):
        t = _group_window(self, group_tail_samples(groups, q), obips)
        assert t.dtype == TREND_DTYPE
        return t


class WorkloadTailRef(node_trend_ref.NodeTrendRef):
    """SG_Q_GROUP_NODES (nc: the row capacity).  window(workload rows, q [N][2], obips) -> NODE_TREND_DTYPE rows (K16's keys)"""

    def window(self, nodes, q, obips):
        return _fold_sides(_workload_window(self, node_tail_samples(nodes, q), obips), len(nodes))
