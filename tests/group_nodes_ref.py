"""References of the workload rows (K16, include/servicegraph.h "workload rows"), of their baselines and of the selection.

group_nodes_ref(group_edges, max_groups, mk, ml): numpy, from a window's group edges (the device's own, or tests/group_ref's).
group_nodes_rows(rows, gmap, max_groups, mk, ml): written apart from it — plain Python ints over the window's ROWS with each ref
replaced by its group ref, *_edges as the number of distinct peers.  The two agree (tests/test_group_nodes_host.py).

The order is ascending group key gk: the groups by id, then the ungrouped KNOWN nodes by id, then LABEL, then OBIP by index — not
ascending by the raw ref word, SG_REF_GROUP being type 3.

The baseline is tests/node_trend_ref.py's window function with the key function swapped for the workload key (wk(ref), side), as
that file swaps K8's: the entry update, expiry, capacity cut and row rule stay K8's code."""
from __future__ import annotations

import types

import numpy as np

from alaz_amd.engine import NODE_DTYPE, NODE_TREND_DTYPE, REF_GROUP, TREND_DTYPE
from tests import node_trend_ref
from tests.group_ref import group_of_ref
from tests.group_trend_ref import workload_keys
from tests.node_trend_ref import node_samples, ref_select_nodes
from tests.nodes_ref import NO_ROW, key_score, score_key

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def gk_of_refs(refs, max_groups: int, mk: int, ml: int) -> np.ndarray:
    """the group key of group refs: g for SG_REF_GROUP | g, else max_groups + K9's node key of the ref"""
    r = np.asarray(refs, dtype=np.uint64)
    t, v = r >> np.uint64(30), r & np.uint64(0x3FFFFFFF)
    base = np.select([t == REF_GROUP, t == 0, t == 1], [0, max_groups, max_groups + mk], max_groups + mk + ml)
    return v + base.astype(np.uint64)


def _side(ge, keys, nodes, out, side):
    if len(ge) == 0:
        return
    pos = np.searchsorted(nodes, keys)
    order = np.argsort(pos, kind="stable")
    ps = pos[order]
    starts = np.flatnonzero(np.concatenate(([True], ps[1:] != ps[:-1])))
    at = ps[starts]
    g = ge[order]
    with np.errstate(over="ignore"):
        out[f"{side}_edges"][at] = np.diff(np.append(starts, len(ps))).astype(np.uint32)
        for f, src in (("count", "count"), ("err", "err_count"), ("sum_ns", "sum_ns"), ("sumsq_us", "sumsq_us"), ("score_q32", "score_q32")):
            out[f"{side}_{f}"][at] = np.add.reduceat(g[src].astype(np.uint64), starts)
        out[f"{side}_max_ns"][at] = np.maximum.reduceat(g["max_ns"].astype(np.uint64), starts)
        out[f"{side}_alive"][at] = np.add.reduceat(g["alive"].astype(np.uint64), starts).astype(np.uint32)
        key = (score_key(g["score_max"]).astype(np.uint64) << np.uint64(32)) | (~g["worst_row"].astype(np.uint64) & np.uint64(M32))
        worst = np.maximum.reduceat(key, starts)
    out[f"{side}_score_max"][at] = key_score((worst >> np.uint64(32)).astype(np.uint32))
    out[f"{side}_worst_row"][at] = (~worst & np.uint64(M32)).astype(np.uint32)


def group_nodes_ref(group_edges: np.ndarray, max_groups: int, mk: int, ml: int) -> np.ndarray:
    """the workload rows of one window's group edges, ascending by group key"""
    ge = group_edges
    if len(ge) == 0:
        return np.zeros(0, dtype=NODE_DTYPE)
    fk, tk = gk_of_refs(ge["from_ref"], max_groups, mk, ml), gk_of_refs(ge["to_ref"], max_groups, mk, ml)
    allk, first = np.unique(np.concatenate([fk, tk]), return_index=True)
    out = np.zeros(len(allk), dtype=NODE_DTYPE)
    out["ref"] = np.concatenate([ge["from_ref"], ge["to_ref"]])[first]
    out["out_worst_row"] = NO_ROW
    out["in_worst_row"] = NO_ROW
    _side(ge, fk, allk, out, "out")
    _side(ge, tk, allk, out, "in")
    o, i = out["out_score_max"], out["in_score_max"]
    out["score"] = np.where(o > i, o, i)
    return out


def _gk_int(gref: int, max_groups: int, mk: int, ml: int) -> int:
    t, v = gref >> 30, gref & 0x3FFFFFFF
    return v if t == REF_GROUP else max_groups + (v if t == 0 else mk + v if t == 1 else mk + ml + v)


def group_nodes_rows(rows: np.ndarray, gmap, max_groups: int, mk: int, ml: int) -> np.ndarray:
    """the same from the window's rows: K9's definition with each ref replaced by its group ref, one row at a time in Python ints;
    *_edges = the number of distinct peers"""
    gmap = np.asarray(gmap, dtype=np.uint32).tolist()
    acc = {}

    def side(gref, s):
        n = acc.setdefault(gref, {"out": None, "in": None})
        if n[s] is None:
            n[s] = dict(peers=set(), count=0, err=0, sum_ns=0, sumsq_us=0, max_ns=0, alive=0, score_q32=0, key=None, worst_row=NO_ROW)
        return n[s]

    for j, r in enumerate(rows):
        f, t = group_of_ref(int(r["from_ref"]), gmap), group_of_ref(int(r["to_ref"]), gmap)
        sc = np.float32(r["score"])
        q = int(np.float64(sc) * 2.0 ** 32) if sc > 0 else 0
        k = int(score_key(np.array([sc], dtype=np.float32))[0])
        for s, me, peer in (("out", f, t), ("in", t, f)):
            a = side(me, s)
            a["peers"].add(peer)
            a["count"] = (a["count"] + int(r["count"])) & M64
            a["err"] = (a["err"] + int(r["err_count"])) & M64
            a["sum_ns"] = (a["sum_ns"] + int(r["sum_ns"])) & M64
            a["sumsq_us"] = (a["sumsq_us"] + int(r["sumsq_us"])) & M64
            a["max_ns"] = max(a["max_ns"], int(r["max_ns"]))
            a["alive"] = (a["alive"] + int(r["alive"])) & M32
            a["score_q32"] = (a["score_q32"] + q) & M64
            if a["key"] is None or k > a["key"]:                       # strictly greater: the first row of a tie stays
                a["key"], a["worst_row"] = k, j
    out = np.zeros(len(acc), dtype=NODE_DTYPE)
    for i, gref in enumerate(sorted(acc, key=lambda x: _gk_int(x, max_groups, mk, ml))):
        out[i]["ref"] = gref
        best = []
        for s in ("out", "in"):
            a = acc[gref][s]
            if a is None:
                out[i][f"{s}_worst_row"] = NO_ROW
                best.append(np.float32(0))
                continue
            out[i][f"{s}_edges"] = len(a["peers"])
            for f in ("count", "err", "sum_ns", "sumsq_us", "max_ns", "alive", "score_q32", "worst_row"):
                out[i][f"{s}_{f}"] = a[f]
            m = key_score(np.array([a["key"]], dtype=np.uint32))[0]
            out[i][f"{s}_score_max"] = m
            best.append(m)
        out[i]["score"] = best[0] if best[0] > best[1] else best[1]
    return out


# ---- the baseline ---------------------------------------------------------------------------------------------------------------
def _keys(s, obips):
    """node_trend_ref's key function with the workload key: (wk(ref), side)"""
    return workload_keys(s["ref"], obips), s["side"].astype(np.uint64)


_window = types.FunctionType(node_trend_ref._window.__code__, {**node_trend_ref._window.__globals__, "row_keys": _keys}, "window")


class GroupNodeTrendRef(node_trend_ref.NodeTrendRef):
    """The workload baseline of one engine (nc: the row capacity).  window(workload rows, obips) -> NODE_TREND_DTYPE rows;
    .entries = the baseline afterwards, from_key = the workload key, to_key = the side."""

    def window(self, nodes, obips):
        t = _window(self, node_samples(nodes), obips)
        assert t.dtype == TREND_DTYPE
        out = np.zeros(len(nodes), dtype=NODE_TREND_DTYPE)
        for side, k in (("in", 0), ("out", 1)):
            h = t[k::2]
            out[f"{side}_lat_dev"], out[f"{side}_err_dev"] = h["lat_dev"], h["err_dev"]
            out[f"{side}_base_mean_us"], out[f"{side}_seen"] = h["base_mean_us"], h["windows_seen"]
        return out


def ref_select_group_nodes(nodes, ntrend, by, k, min_value):
    """row positions K7 selects from the workload rows by key `by` (a key of engine.NSEL_BY): the node selection's rule"""
    return ref_select_nodes(nodes, ntrend, by, k, min_value)
