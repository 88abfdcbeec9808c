"""Pure-Python reference of the workload contraction (K14, include/servicegraph.h "groups"): a window's rows (replay.EDGE_OUT_DTYPE,
canonical order) and a group map -> its group edges (engine.GROUP_EDGE_DTYPE), row_group and perm, exactly as the device computes
them.  Python ints and one dict entry per (group key of from, group key of to); nothing here sorts more than the dict's keys."""
from __future__ import annotations

import numpy as np

from alaz_amd.engine import GROUP_EDGE_DTYPE, NO_GROUP, REF_GROUP

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
KNOWN, LABEL, OBIP = 0, 1, 2


def node_key(ref: int, max_known: int, max_labels: int) -> int:
    """K9's node key of a ref"""
    t, v = ref >> 30, ref & 0x3FFFFFFF
    return v if t == KNOWN else max_known + v if t == LABEL else max_known + max_labels + v


def group_key(ref: int, gmap, max_groups: int, max_known: int, max_labels: int) -> int:
    t, v = ref >> 30, ref & 0x3FFFFFFF
    if t == KNOWN and v < len(gmap) and int(gmap[v]) != NO_GROUP:
        return int(gmap[v])
    return max_groups + node_key(ref, max_known, max_labels)


def group_of_ref(ref: int, gmap) -> int:
    t, v = ref >> 30, ref & 0x3FFFFFFF
    if t == KNOWN and v < len(gmap) and int(gmap[v]) != NO_GROUP:
        return (REF_GROUP << 30) | int(gmap[v])
    return ref


def key_score(k: int) -> np.float32:
    b = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & M32)
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def group_ref(rows: np.ndarray, gmap, max_groups: int, max_known: int, max_labels: int):
    """(group edges, row_group, perm) of one window's rows under the map gmap (u32 per KNOWN id, NO_GROUP = none)"""
    E = len(rows)
    gmap = np.asarray(gmap, dtype=np.uint32).tolist()
    col = {f: rows[f].tolist() for f in ("from_ref", "to_ref", "count", "err_count", "sum_ns", "sumsq_us", "max_ns", "alive")}
    score = np.ascontiguousarray(rows["score"], dtype=np.float32)
    bits, val = score.view(np.uint32).tolist(), score.tolist()        # (a float32 is exact as a Python float)
    fr, to = col["from_ref"], col["to_ref"]
    runs = {}
    for j in range(E):
        k = (group_key(fr[j], gmap, max_groups, max_known, max_labels), group_key(to[j], gmap, max_groups, max_known, max_labels))
        runs.setdefault(k, []).append(j)                              # (row order: the third sort key)
    out = np.zeros(len(runs), dtype=GROUP_EDGE_DTYPE)
    row_group = np.zeros(E, dtype=np.uint32)
    perm = np.zeros(E, dtype=np.uint32)
    at = 0
    for i, k in enumerate(sorted(runs)):
        js = runs[k]
        o = out[i]
        cnt = err = sm = ssq = mx = q32 = alive = 0
        worst = -1
        fnodes, prev = 0, None
        for j in js:
            cnt += col["count"][j]; err += col["err_count"][j]; sm += col["sum_ns"][j]; ssq += col["sumsq_us"][j]
            mx = max(mx, col["max_ns"][j]); alive += col["alive"][j]
            if val[j] > 0:
                q32 += int(val[j] * 2.0 ** 32)
            b = bits[j]
            worst = max(worst, (((~b & M32) if b & 0x80000000 else b | 0x80000000) << 32) | (~j & M32))
            if prev is None or fr[j] != prev:                         # the position before it in perm has another from_ref
                fnodes += 1
            prev = fr[j]
            row_group[j] = i
        perm[at:at + len(js)] = js
        o["count"], o["err_count"], o["sum_ns"], o["sumsq_us"], o["max_ns"], o["score_q32"] = cnt & M64, err & M64, sm & M64, ssq & M64, mx, q32 & M64
        o["from_ref"] = group_of_ref(fr[js[0]], gmap)
        o["to_ref"] = group_of_ref(to[js[0]], gmap)
        o["edges"], o["from_nodes"], o["first"], o["alive"] = len(js), fnodes, at, alive & M32
        o["worst_row"] = ~worst & M32
        o["score_max"] = key_score(worst >> 32)
        at += len(js)
    return out, row_group, perm
