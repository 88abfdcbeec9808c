"""numpy reference of the per-node baselines (K10, include/servicegraph.h "node baselines") and of the node selection.

A window's node rows (tests/nodes_ref.nodes_ref of its rows) become 2N samples, sample 2k + s for node row k and side s (0 in, 1
out), with key (nk, s): nk is K8's key word of the node's ref.  They run through tests/trend_ref.TrendRef's own update — its window
function is called with two of its module globals swapped for the node forms (the samples of a side, the keys of a sample), so the
entry update, expiry, capacity cut and row rule are K8's code, not a copy — and the per-sample trend rows fold into one
NODE_TREND_DTYPE row per node."""
import types

import numpy as np

from alaz_amd.engine import NODE_TREND_DTYPE, TREND_DTYPE
from tests import trend_ref
from tests.select_by_ref import ref_select_by

#: one sample of the node baseline: the node's ref, its side, and that side's count, errors and latency sum (u64 each)
SAMPLE_DTYPE = np.dtype([("ref", "<u4"), ("side", "<u4"), ("count", "<u8"), ("err", "<u8"), ("sum_ns", "<u8")])


def node_samples(nodes):
    """the 2N samples of a window's node rows, in key order"""
    s = np.zeros(2 * len(nodes), dtype=SAMPLE_DTYPE)
    s["ref"] = np.repeat(nodes["ref"], 2)
    s["side"] = np.tile(np.array([0, 1], np.uint32), len(nodes))
    for side, k in (("in", 0), ("out", 1)):
        s["count"][k::2] = nodes[f"{side}_count"]
        s["err"][k::2] = nodes[f"{side}_err"]
        s["sum_ns"][k::2] = nodes[f"{side}_sum_ns"]
    return s


def x_err(err, count):
    """floor(err * 2^20 / count), exact (Python integers: no u64 overflow), as fp64"""
    return np.array([float((int(e) << 20) // int(c)) if c else 0.0 for e, c in zip(err, count)], dtype=np.float64)


def _samples(s):
    """trend_ref.samples for node samples: (live, x_lat, x_err)"""
    cnt = s["count"].astype(np.uint64)
    live = cnt > 0
    c = np.where(live, cnt, np.uint64(1))
    xl = np.minimum(s["sum_ns"].astype(np.uint64) // c, np.uint64(1 << 52)).astype(np.float64)
    return live, xl, x_err(s["err"], cnt)


def _keys(s, obips):
    """trend_ref.row_keys for node samples: (nk, side)"""
    return trend_ref.ref_keys(s["ref"], obips), s["side"].astype(np.uint64)


_window = types.FunctionType(trend_ref.TrendRef.window.__code__, {**vars(trend_ref), "samples": _samples, "row_keys": _keys},
                             "window")


class NodeTrendRef(trend_ref.TrendRef):
    """The node baseline of one engine.  window(nodes, obips) -> the window's NODE_TREND_DTYPE rows; .entries = the baseline."""

    def __init__(self, ncap, shift=4, warmup=4, ttl=64, max_entries=0, lat_floor_ns=1000, err_floor=10486):
        super().__init__(1, shift, warmup, ttl, max_entries or min(1 << 31, 4 * max(ncap, 1)), lat_floor_ns, err_floor)

    def window(self, nodes, obips):
        t = _window(self, node_samples(nodes), obips)
        assert t.dtype == TREND_DTYPE
        out = np.zeros(len(nodes), dtype=NODE_TREND_DTYPE)
        for side, k in (("in", 0), ("out", 1)):
            h = t[k::2]
            out[f"{side}_lat_dev"], out[f"{side}_err_dev"] = h["lat_dev"], h["err_dev"]
            out[f"{side}_base_mean_us"], out[f"{side}_seen"] = h["base_mean_us"], h["windows_seen"]
        return out


def ref_select_nodes(nodes, ntrend, by, k, min_value):
    """node positions K7 selects from `nodes` by key `by` (a key of engine.NSEL_BY), with ntrend the window's NODE_TREND_DTYPE rows
    (None for by = "score")"""
    if by == "new":
        seen = np.zeros(len(nodes), dtype=TREND_DTYPE)
        seen["windows_seen"] = ntrend["in_seen"] | ntrend["out_seen"]
        req = np.zeros(len(nodes), dtype=[("count", "<u4")])
        req["count"] = (nodes["in_count"] | nodes["out_count"]) != 0
        return ref_select_by(req, seen, "new", k, min_value)
    v = nodes["score"] if by == "score" else ntrend[by]
    vals = np.zeros(len(nodes), dtype=[("v", "<f4")])
    vals["v"] = v
    return ref_select_by(None, vals, "v", k, min_value)
