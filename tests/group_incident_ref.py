"""Pure-Python reference of the workload incidents (K18, include/servicegraph.h "workload incidents").

group_incident_ref(groups, gnodes, by, min_value, trend=None, rank=None) runs the contract over a window's group edges and workload
rows (numpy structured arrays as window_groups() and window_group_nodes() return them) and, for a trend key, the group trend rows
(window_group_trend()), with a union-find over ROW POSITIONS and every sum in Python ints; rank: the window's workload rank rows
(window_group_rank()) when K17 was on.  It returns (INCIDENT_DTYPE rows, the incident per workload row).  Every field is an integer
sum, an integer max or a max of order-preserving float bits: the device result must equal it byte for byte.

The sums are the group edge's own fields (count, err_count, sum_ns, score_q32) as they stand: rows folded into a red group edge
count whether or not they would be red themselves.  worst_row is a GROUP-EDGE index."""
import numpy as np

from alaz_amd.engine import INCIDENT_DTYPE, NO_INCIDENT, SEL_BY
from tests.nodes_ref import score_key

U64 = (1 << 64) - 1
BY = {**{k: v for k, v in SEL_BY.items()}, 0: 0, 1: 1, 2: 2}


def group_values(groups, by, trend=None):
    """float32 value per group edge: score_max, or the group edge's lat_dev / err_dev of the window's group trend rows"""
    by = BY[by]
    if by == 0:
        return np.ascontiguousarray(groups["score_max"], dtype=np.float32)
    assert trend is not None and len(trend) == len(groups), "a trend key needs the window's group trend rows"
    return np.ascontiguousarray(trend["lat_dev" if by == 1 else "err_dev"], dtype=np.float32)


def red_groups(groups, gnodes, by, min_value, trend=None):
    """(values, red mask, source row position, destination row position); a group edge whose from_ref or to_ref has no workload
    row is never red"""
    val = group_values(groups, by, trend)
    pos = {int(r): v for v, r in enumerate(gnodes["ref"])}
    src = np.array([pos.get(int(x), -1) for x in groups["from_ref"]], dtype=np.int64)
    dst = np.array([pos.get(int(x), -1) for x in groups["to_ref"]], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        red = (val >= np.float32(min_value)) & (src >= 0) & (dst >= 0)  # (NaN never)
    return val, red, src, dst


def group_incident_ref(groups, gnodes, by="score", min_value=0.0, trend=None, rank=None):
    n = len(gnodes)
    val, red, src, dst = red_groups(groups, gnodes, by, min_value, trend)
    parent = list(range(n))
    flag = [False] * n

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for j in np.flatnonzero(red):
        u, v = int(src[j]), int(dst[j])
        flag[u] = flag[v] = True
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)                              # (min-hooking: a root is its component's smallest row)
    heads = [v for v in range(n) if flag[v] and find(v) == v]          # ascending: incident i's first_node is heads[i]
    number = {v: i for i, v in enumerate(heads)}
    node_inc = np.full(n, NO_INCIDENT, dtype=np.uint32)
    out = np.zeros(len(heads), dtype=INCIDENT_DTYPE)
    acc = [dict(count=0, err=0, sum_ns=0, score_q32=0, rank_sum=0, nodes=0, edges=0, worst=None, top=None, culprit=None) for _ in heads]
    nkey = score_key(gnodes["score"]) if n else []
    for v in range(n):
        if not flag[v]:
            continue
        i = number[find(v)]
        node_inc[v] = i
        a = acc[i]
        a["nodes"] += 1
        k = (int(nkey[v]), -v)
        if a["top"] is None or k > a["top"]:
            a["top"] = k
        if rank is not None:
            r = int(rank["rank"][v])
            a["rank_sum"] = (a["rank_sum"] + r) & U64
            if a["culprit"] is None or (r, -v) > a["culprit"]:
                a["culprit"] = (r, -v)
    vkey = score_key(val) if len(groups) else []
    for j in np.flatnonzero(red):
        j = int(j)
        a = acc[int(node_inc[src[j]])]
        assert node_inc[src[j]] == node_inc[dst[j]]
        a["edges"] += 1
        a["count"] = (a["count"] + int(groups["count"][j])) & U64
        a["err"] = (a["err"] + int(groups["err_count"][j])) & U64
        a["sum_ns"] = (a["sum_ns"] + int(groups["sum_ns"][j])) & U64
        a["score_q32"] = (a["score_q32"] + int(groups["score_q32"][j])) & U64
        k = (int(vkey[j]), -j)
        if a["worst"] is None or k > a["worst"]:
            a["worst"] = k
    for i, a in enumerate(acc):
        o = out[i]
        for f in ("count", "err", "sum_ns", "score_q32", "rank_sum", "nodes", "edges"):
            o[f] = a[f]
        o["first_node"] = heads[i]
        o["worst_row"] = -a["worst"][1]
        o["value_max"] = val[-a["worst"][1]]
        o["top_node"] = -a["top"][1]
        o["culprit_node"] = -a["culprit"][1] if rank is not None else NO_INCIDENT
    return out, node_inc
