"""Pure-Python reference of the workload ranking (K17, include/servicegraph.h "workload ranking").

group_rank_ref(groups, gnodes, ...) runs the contract over a window's group edges and workload rows (numpy structured arrays as
window_groups() and window_group_nodes() return them: groups need from_ref, to_ref, edges, score_q32; gnodes need ref, score) in
Python ints, asserts the contract's invariants on every iteration (sum r' == sum R + sum m; sum r <= M; t_u * w_j <= m_u < 2^56)
and returns RANK_DTYPE rows.  Integer arithmetic only: the device result must equal it byte for byte.  The selection over the rows
is K11's (tests/rank_ref.py ref_select_rank)."""
import numpy as np

from alaz_amd.engine import RANK_DTYPE
from tests.rank_ref import M, SEEDS, U64, q16


def group_weight(edges, score_q32):
    """w = edges + min(score_q32 >> 16, 65536 * edges)"""
    edges, q = int(edges), int(score_q32)
    return edges + min(q >> 16, 65536 * edges)


def group_rank_ref(groups, gnodes, iters=0, damping_q8=0, seed="score", seed_min_score=0.0, trace=None, no_key=()):
    """no_key: refs that have no group key (a ref beyond the id spaces): a group edge that names one carries w = 0"""
    iters = iters or 20
    D = damping_q8 or 218
    assert 1 <= iters <= 64 and 1 <= D <= 255
    seed = SEEDS[seed]
    n = len(gnodes)
    out = np.zeros(n, dtype=RANK_DTYPE)
    if n == 0:
        return out
    pos = {int(r): v for v, r in enumerate(gnodes["ref"])}
    assert len(pos) == n
    src, dst, w = [], [], []
    for f, t, e, q in zip(groups["from_ref"], groups["to_ref"], groups["edges"], groups["score_q32"]):
        if int(f) in no_key or int(t) in no_key:
            src.append(0); dst.append(0); w.append(0)
            continue
        src.append(pos[int(f)]); dst.append(pos[int(t)])             # (a KeyError: a group edge names a workload K16 does not have)
        w.append(group_weight(e, q))
        assert w[-1] <= 65537 * int(e)
    W = [0] * n
    for u, x in zip(src, w):
        W[u] += x
    assert max(W, default=0) < U64
    smin = np.float32(seed_min_score)
    if seed == 0:
        a = [q16(s) if np.float32(s) >= smin else 0 for s in gnodes["score"]]
    else:
        a = [1] * n
    A = sum(a)
    if A == 0:
        a, A = [1] * n, n
    fa = M // A
    p = [x * fa for x in a]
    R = [(x >> 8) * (256 - D) for x in p]
    r = list(p)
    assert sum(r) <= M
    for _ in range(iters):
        m = [(x >> 8) * D for x in r]
        t = [mu // Wu if Wu else 0 for mu, Wu in zip(m, W)]
        nr = [Rv + (mv - tv * Wv) for Rv, mv, tv, Wv in zip(R, m, t, W)]
        for u, v, x in zip(src, dst, w):
            h = t[u] * x
            assert h <= m[u] < M
            nr[v] += h
        assert sum(nr) == sum(R) + sum(m), "mass"
        assert sum(nr) <= M and max(nr) <= M
        r = nr
        if trace is not None:
            trace.append(list(r))
    out["rank"] = np.array(r, dtype=np.uint64)
    out["ref"] = gnodes["ref"]
    out["share"] = (out["rank"].astype(np.float64) * 2.0 ** -56).astype(np.float32)
    return out


def seed_sum(gnodes, seed="score", seed_min_score=0.0):
    """A before the fallback: 0 means the window fell back to the uniform seed"""
    if SEEDS[seed] == 1:
        return len(gnodes)
    smin = np.float32(seed_min_score)
    return sum(q16(s) if np.float32(s) >= smin else 0 for s in gnodes["score"])
