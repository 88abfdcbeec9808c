"""numpy reference of the node rollup (K9, include/servicegraph.h "node rollup"): a window's rows (replay.EDGE_OUT_DTYPE, canonical
order) -> its node rows (engine.NODE_DTYPE), exactly as the device computes them.

A ref is type << 30 | value, so ascending (type, value) is ascending ref.  Every field is an integer sum (wrapping u64), an integer
max or the max of the 64-bit key (order-preserving score key << 32 | ~row): the largest score, then the smallest row."""
from __future__ import annotations

import numpy as np

from alaz_amd.engine import NODE_DTYPE

NO_ROW = 0xFFFFFFFF


def score_key(score: np.ndarray) -> np.ndarray:
    """order-preserving u32 key of float32 scores (+0.0 above -0.0)"""
    b = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_score(key: np.ndarray) -> np.ndarray:
    k = np.asarray(key, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return b.view(np.float32)


def score_q32(score: np.ndarray) -> np.ndarray:
    """(uint64)((double)score * 2^32) per row; a score that is not > 0 adds 0"""
    s = np.asarray(score, dtype=np.float32)
    pos = s > 0
    out = np.zeros(len(s), dtype=np.uint64)
    out[pos] = (s[pos].astype(np.float64) * 2.0 ** 32).astype(np.uint64)
    return out


def _side(rows: np.ndarray, refs: np.ndarray, nodes: np.ndarray, out: np.ndarray, side: str):
    if len(rows) == 0:
        return
    pos = np.searchsorted(nodes, refs)
    order = np.argsort(pos, kind="stable")
    ps = pos[order]
    starts = np.flatnonzero(np.concatenate(([True], ps[1:] != ps[:-1])))
    at = ps[starts]
    r = rows[order]
    j = order.astype(np.uint64)
    with np.errstate(over="ignore"):
        out[f"{side}_edges"][at] = np.diff(np.append(starts, len(ps))).astype(np.uint32)
        out[f"{side}_count"][at] = np.add.reduceat(r["count"].astype(np.uint64), starts)
        out[f"{side}_err"][at] = np.add.reduceat(r["err_count"].astype(np.uint64), starts)
        out[f"{side}_sum_ns"][at] = np.add.reduceat(r["sum_ns"].astype(np.uint64), starts)
        out[f"{side}_sumsq_us"][at] = np.add.reduceat(r["sumsq_us"].astype(np.uint64), starts)
        out[f"{side}_max_ns"][at] = np.maximum.reduceat(r["max_ns"].astype(np.uint64), starts)
        out[f"{side}_alive"][at] = np.add.reduceat(r["alive"].astype(np.uint64), starts).astype(np.uint32)
        out[f"{side}_score_q32"][at] = np.add.reduceat(score_q32(r["score"]), starts)
        key = (score_key(r["score"]).astype(np.uint64) << np.uint64(32)) | (~j & np.uint64(0xFFFFFFFF))
        worst = np.maximum.reduceat(key, starts)
    out[f"{side}_score_max"][at] = key_score((worst >> np.uint64(32)).astype(np.uint32))
    out[f"{side}_worst_row"][at] = (~worst & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def nodes_ref(rows: np.ndarray) -> np.ndarray:
    """the node rows of one window's rows"""
    if len(rows) == 0:
        return np.zeros(0, dtype=NODE_DTYPE)
    fr, to = rows["from_ref"].astype(np.uint32), rows["to_ref"].astype(np.uint32)
    nodes = np.unique(np.concatenate([fr, to]))
    out = np.zeros(len(nodes), dtype=NODE_DTYPE)
    out["ref"] = nodes
    out["out_worst_row"] = NO_ROW
    out["in_worst_row"] = NO_ROW
    _side(rows, fr, nodes, out, "out")
    _side(rows, to, nodes, out, "in")
    o, i = out["out_score_max"], out["in_score_max"]
    out["score"] = np.where(o > i, o, i)
    return out


def nodes_loop(rows: np.ndarray) -> np.ndarray:
    """the same, one row at a time in plain Python (the cross-check of nodes_ref)"""
    acc = {}
    M = (1 << 64) - 1

    def side(ref, s):
        n = acc.setdefault(int(ref), {"out": None, "in": None})
        if n[s] is None:
            n[s] = dict(edges=0, count=0, err=0, sum_ns=0, sumsq_us=0, max_ns=0, alive=0, score_q32=0, score_max=None, worst_row=NO_ROW)
        return n[s]

    for j, r in enumerate(rows):
        sc = float(r["score"])
        q = int(np.float64(np.float32(sc)) * 2.0 ** 32) if sc > 0 else 0
        for s, ref in (("out", r["from_ref"]), ("in", r["to_ref"])):
            a = side(ref, s)
            a["edges"] += 1
            a["count"] = (a["count"] + int(r["count"])) & M
            a["err"] = (a["err"] + int(r["err_count"])) & M
            a["sum_ns"] = (a["sum_ns"] + int(r["sum_ns"])) & M
            a["sumsq_us"] = (a["sumsq_us"] + int(r["sumsq_us"])) & M
            a["max_ns"] = max(a["max_ns"], int(r["max_ns"]))
            a["alive"] += int(r["alive"])
            a["score_q32"] = (a["score_q32"] + q) & M
            k = int(score_key(np.array([r["score"]], dtype=np.float32))[0])
            if a["score_max"] is None or k > a["score_max"]:           # strictly greater: the first row of a tie stays
                a["score_max"], a["worst_row"] = k, j
    out = np.zeros(len(acc), dtype=NODE_DTYPE)
    for i, ref in enumerate(sorted(acc)):
        out[i]["ref"] = ref
        best = []
        for s in ("out", "in"):
            a = acc[ref][s]
            if a is None:
                out[i][f"{s}_worst_row"] = NO_ROW
                best.append(np.float32(0))
                continue
            for f in ("edges", "count", "err", "sum_ns", "sumsq_us", "max_ns", "alive", "score_q32", "worst_row"):
                out[i][f"{s}_{f}"] = a[f]
            m = key_score(np.array([a["score_max"]], dtype=np.uint32))[0]
            out[i][f"{s}_score_max"] = m
            best.append(m)
        out[i]["score"] = best[0] if best[0] > best[1] else best[1]
    return out
