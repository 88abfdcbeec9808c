"""Pure-Python reference of the workload impact (K22, include/servicegraph.h "workload impact").

impact_ref(groups, gnodes, n_incidents, node_inc, max_incidents, max_hops) runs the contract over a window's group edges, workload
rows, incident count and incident per workload row (numpy arrays as window_groups(), window_group_nodes(),
len(window_group_incidents()) and window_group_node_incident() return them): one breadth-first search per covered incident against
the call edges, every sum in Python ints.  It returns (impact rows (n, 8) <u8, hops per workload row <u4, mask rows (rows, W) <u8).
Every value is an integer sum or the max of a key: the device result must equal it byte for byte."""
import numpy as np

from alaz_amd.engine import IMPACT_WORDS, NO_HOPS

U64 = (1 << 64) - 1
NOTHING_FAR = 0x00000000FFFFFFFF


def call_edges(groups, gnodes):
    """[(from row, to row, count, err_count)] of the group edges that are call edges: count > 0, both refs have workload rows, and
    the rows differ"""
    pos = {int(r): v for v, r in enumerate(gnodes["ref"])}
    out = []
    for j in range(len(groups)):
        c = int(groups["count"][j])
        u, v = pos.get(int(groups["from_ref"][j]), -1), pos.get(int(groups["to_ref"][j]), -1)
        if c > 0 and u >= 0 and v >= 0 and u != v:
            out.append((u, v, c, int(groups["err_count"][j])))
    return out


def impact_ref(groups, gnodes, n_incidents, node_inc, max_incidents, max_hops):
    n = len(gnodes)
    inc = [int(x) for x in node_inc]
    assert len(inc) == n
    cov = min(int(n_incidents), int(max_incidents))
    W = (int(max_incidents) + 63) // 64
    edges = call_edges(groups, gnodes)
    callers = [[] for _ in range(n)]                                   # callers[v]: the rows u with a call edge u -> v
    arrives = [False] * n
    for u, v, _, _ in edges:
        callers[v].append(u)
        arrives[v] = True
    rows = np.zeros((cov, IMPACT_WORDS), dtype="<u8")
    hops = [NO_HOPS] * n
    mask = [[0] * W for _ in range(n)]
    for i in range(cov):
        dist = {v: 0 for v in range(n) if inc[v] == i}
        frontier = sorted(dist)
        for r in range(1, int(max_hops) + 1):
            nxt = set()
            for v in frontier:
                for u in callers[v]:
                    if u not in dist:
                        nxt.add(u)
            for u in nxt:
                dist[u] = r
            frontier = sorted(nxt)
            if not frontier:
                break
        exposed = [v for v, d in dist.items() if d >= 1]
        far = NOTHING_FAR
        if exposed:
            h = max(dist[v] for v in exposed)
            far = h << 32 | min(v for v in exposed if dist[v] == h)
        entries = [v for v in dist if not arrives[v]]
        into = [(c, e) for u, v, c, e in edges if inc[v] == i and inc[u] != i]
        rows[i] = [len(exposed), sum(1 for v in exposed if dist[v] == 1), far, len(entries),
                   sum(int(gnodes["out_count"][v]) for v in entries) & U64, sum(int(gnodes["out_err"][v]) for v in entries) & U64,
                   sum(c for c, _ in into) & U64, sum(e for _, e in into) & U64]
        for v, d in dist.items():
            hops[v] = min(hops[v], d)
            mask[v][i >> 6] |= 1 << (i & 63)
    return rows, np.array(hops, dtype="<u4"), np.array(mask, dtype="<u8").reshape(n, W)
