"""Pure-Python reference of the incidents (K12, include/servicegraph.h "incidents").

incident_ref(rows, nodes, by, min_value, trend=None, rank=None) runs the contract over a window's edge rows, node rows and, for a
trend key, trend rows (numpy structured arrays as the engine returns them) with a union-find over the node rows and every sum in
Python ints; rank: the window's rank rows when the ranking was on.  It returns (INCIDENT_DTYPE rows, the incident per node row).
Every field is an integer sum, an integer max or a max of order-preserving float bits: the device result must equal it byte for
byte."""
import numpy as np

from alaz_amd.engine import INCIDENT_DTYPE, NO_INCIDENT, SEL_BY
from tests.nodes_ref import score_key, score_q32

U64 = (1 << 64) - 1
BY = {**{k: v for k, v in SEL_BY.items()}, 0: 0, 1: 1, 2: 2}


def row_values(rows, by, trend=None):
    """float32 value per row: the score, or the row's lat_dev / err_dev of the window's trend rows"""
    by = BY[by]
    if by == 0:
        return np.ascontiguousarray(rows["score"], dtype=np.float32)
    assert trend is not None and len(trend) == len(rows), "a trend key needs the window's trend rows"
    return np.ascontiguousarray(trend["lat_dev" if by == 1 else "err_dev"], dtype=np.float32)


def red_rows(rows, nodes, by, min_value, trend=None):
    """(values, red mask, source node row, destination node row); a row whose from_ref or to_ref has no node row is never red"""
    val = row_values(rows, by, trend)
    pos = {int(r): v for v, r in enumerate(nodes["ref"])}
    src = np.array([pos.get(int(x), -1) for x in rows["from_ref"]], dtype=np.int64)
    dst = np.array([pos.get(int(x), -1) for x in rows["to_ref"]], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        red = (val >= np.float32(min_value)) & (src >= 0) & (dst >= 0)  # (NaN never)
    return val, red, src, dst


def incident_ref(rows, nodes, by="score", min_value=0.0, trend=None, rank=None):
    n = len(nodes)
    val, red, src, dst = red_rows(rows, nodes, by, min_value, trend)
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
            parent[max(a, b)] = min(a, b)                              # (min-hooking: a root is its component's smallest node)
    node_inc = np.full(n, NO_INCIDENT, dtype=np.uint32)
    number = {}
    for v in range(n):
        if flag[v] and find(v) == v:
            number[v] = len(number)
    out = np.zeros(len(number), dtype=INCIDENT_DTYPE)
    acc = [dict(count=0, err=0, sum_ns=0, score_q32=0, rank_sum=0, nodes=0, edges=0, worst=None, top=None, culprit=None) for _ in number]
    nkey = score_key(nodes["score"]) if n else []
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
    vkey = score_key(val) if len(rows) else []
    q32 = score_q32(rows["score"]) if len(rows) else []
    for j in np.flatnonzero(red):
        j = int(j)
        a = acc[int(node_inc[src[j]])]
        assert node_inc[src[j]] == node_inc[dst[j]]
        a["edges"] += 1
        a["count"] = (a["count"] + int(rows["count"][j])) & U64
        a["err"] = (a["err"] + int(rows["err_count"][j])) & U64
        a["sum_ns"] = (a["sum_ns"] + int(rows["sum_ns"][j])) & U64
        a["score_q32"] = (a["score_q32"] + int(q32[j])) & U64
        k = (int(vkey[j]), -j)
        if a["worst"] is None or k > a["worst"]:
            a["worst"] = k
    first = sorted(number, key=number.get)
    for i, a in enumerate(acc):
        o = out[i]
        for f in ("count", "err", "sum_ns", "score_q32", "rank_sum", "nodes", "edges"):
            o[f] = a[f]
        o["first_node"] = first[i]
        o["worst_row"] = -a["worst"][1]
        o["value_max"] = val[-a["worst"][1]]
        o["top_node"] = -a["top"][1]
        o["culprit_node"] = -a["culprit"][1] if rank is not None else NO_INCIDENT
    return out, node_inc


#: the score quantiles at which the GPU tests put the threshold (beside -inf and +inf); tests/test_incident_host.py asserts on the
#: oracle's rows of the same windows what they cover: windows of one incident, of more than 3, and incidents of 3 nodes and more
QUANTILES = (0.0, 0.5, 0.9, 0.99)


def quantile_threshold(values, q):
    """the float32 value at quantile q of `values` (NaN left out; the element at floor(q * (n - 1)) of the sorted values)"""
    v = np.sort(np.asarray(values, dtype=np.float32)[~np.isnan(values)])
    return float(v[int(q * (len(v) - 1))]) if len(v) else 0.0
