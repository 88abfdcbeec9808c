"""Pure-Python reference of the culprit ranking (K11, include/servicegraph.h "culprit ranking") and of its selection.

rank_ref(rows, nodes, ...) runs the contract over a window's edge rows and node rows (numpy structured arrays as the engine returns
them: rows need from_ref, to_ref, score; nodes need ref, score) in Python ints, asserts the contract's invariants on every
iteration (sum r' == sum R + sum m; sum r <= M; every product below 2^64) and returns RANK_DTYPE rows.  Integer arithmetic only:
the device result must equal it byte for byte."""
import numpy as np

from alaz_amd.engine import RANK_DTYPE

M = 1 << 56
U64 = 1 << 64
SEEDS = {"score": 0, "uniform": 1, 0: 0, 1: 1}


def q16(s):
    """q16 of a float32 score: s > 0 ? min((uint32_t)(s * 65536.0f), 65536) : 0 (NaN: 0)"""
    s = np.float32(s)
    if not s > 0:
        return 0
    if s >= 1:
        return 65536
    return int(np.float32(s * np.float32(65536.0)))                   # (a product by a power of two is exact; int() truncates)


def rank_ref(rows, nodes, iters=0, damping_q8=0, seed="score", seed_min_score=0.0, trace=None):
    iters = iters or 20
    D = damping_q8 or 218
    assert 1 <= iters <= 64 and 1 <= D <= 255
    seed = SEEDS[seed]
    n = len(nodes)
    out = np.zeros(n, dtype=RANK_DTYPE)
    if n == 0:
        return out
    pos = {int(r): v for v, r in enumerate(nodes["ref"])}
    assert len(pos) == n
    src = [pos[int(x)] for x in rows["from_ref"]]                     # (a KeyError: a row names a node the rollup does not have)
    dst = [pos[int(x)] for x in rows["to_ref"]]
    w = [1 + q16(s) for s in rows["score"]]
    W = [0] * n
    for u, x in zip(src, w):
        W[u] += x
    assert max(W, default=0) < U64
    smin = np.float32(seed_min_score)
    if seed == 0:
        a = [q16(s) if np.float32(s) >= smin else 0 for s in nodes["score"]]
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
    for it in range(iters):
        m = [(x >> 8) * D for x in r]
        t = [mu // Wu if Wu else 0 for mu, Wu in zip(m, W)]
        nr = [Rv + (mv - tv * Wv) for Rv, mv, tv, Wv in zip(R, m, t, W)]
        for u, v, x in zip(src, dst, w):
            h = t[u] * x
            assert h <= m[u] < U64
            nr[v] += h
        assert sum(nr) == sum(R) + sum(m), "mass"
        assert sum(nr) <= M and max(nr) <= M
        r = nr
        if trace is not None:
            trace.append(list(r))
    out["rank"] = np.array(r, dtype=np.uint64)
    out["ref"] = nodes["ref"]
    out["share"] = (out["rank"].astype(np.float64) * 2.0 ** -56).astype(np.float32)
    return out


def rank_keys(rank_rows, min_share=float("-inf")):
    """the K7 key of every rank row: min(rank >> 24, 0xFFFFFFFF) where share >= min_share (a float32 comparison, NaN never), else 0"""
    k = np.minimum(rank_rows["rank"] >> np.uint64(24), np.uint64(0xFFFFFFFF)).astype(np.uint64)
    with np.errstate(invalid="ignore"):
        ok = rank_rows["share"] >= np.float32(min_share)
    return np.where(ok, k, np.uint64(0))


def ref_select_rank(rank_rows, k, min_share=float("-inf")):
    """node positions K7 selects from the rank rows: k = 0 every candidate (key > 0) in node order, else the k largest keys,
    descending, ties by node position"""
    key = rank_keys(rank_rows, min_share)
    cand = np.flatnonzero(key > 0)
    if k == 0:
        return cand.astype(np.uint32)
    order = sorted(cand.tolist(), key=lambda i: (-int(key[i]), i))
    return np.array(order[:k], dtype=np.uint32)
