"""numpy reference of the latency percentiles (K20; include/servicegraph.h, "latency percentiles"): the three folds of the rows'
histograms and the quantile Q.  Everything is computed from what an engine returns for a window: window_hist(), the rows,
window_nodes(), window_groups(), window_group_perm() and window_group_nodes()."""
import numpy as np

BINS = 16


def quantile(bins, max_ns: int, qm: int) -> int:
    """Q(B, max_ns, qm) in Python integers"""
    b = [int(x) for x in bins]
    total = sum(b)
    if total == 0:
        return 0
    rank = max(1, (total // 1000) * qm + -((total % 1000) * qm // -1000))
    cum, k = 0, BINS - 1
    for i, x in enumerate(b):
        cum += x
        if cum >= rank:
            k = i
            break
    edge = int(max_ns) if k == BINS - 1 else 1 << (17 + k)
    edge = min(edge, int(max_ns))
    return min(edge // 1000, 0xFFFFFFFF)


def quantiles(hist, max_ns, permille) -> np.ndarray:
    """hist [..., 16], max_ns [...] -> [..., n_q] u32"""
    hist = np.asarray(hist, dtype=np.uint64)
    max_ns = np.asarray(max_ns, dtype=np.uint64)
    flat, mx = hist.reshape(-1, BINS), max_ns.reshape(-1)
    out = np.zeros((len(flat), len(permille)), dtype=np.uint32)
    for i in range(len(flat)):
        for j, qm in enumerate(permille):
            out[i, j] = quantile(flat[i], mx[i], int(qm))
    return out.reshape(hist.shape[:-1] + (len(permille),))


def _positions(refs, keys) -> np.ndarray:
    """the position in refs (unique) of every key; every key is one of them"""
    order = np.argsort(refs, kind="stable")
    at = order[np.searchsorted(refs[order], keys)] if len(refs) else np.zeros(len(keys), dtype=np.int64)
    assert np.array_equal(refs[at], keys)
    return at


def _fold_sides(hist, from_ref, to_ref, ent_ref) -> np.ndarray:
    out = np.zeros((len(ent_ref), 2, BINS), dtype=np.uint64)
    if len(from_ref):
        h = np.asarray(hist, dtype=np.uint64)
        np.add.at(out[:, 0, :], _positions(ent_ref, from_ref), h)
        np.add.at(out[:, 1, :], _positions(ent_ref, to_ref), h)
    return out


def fold_nodes(hist, rows, nodes) -> np.ndarray:
    """[nodes][2][16] u64: out side, in side"""
    return _fold_sides(hist[: len(rows)], rows["from_ref"], rows["to_ref"], nodes["ref"])


def row_group(groups, perm) -> np.ndarray:
    """the group edge of every row, from the runs perm[first .. first + edges)"""
    rg = np.zeros(len(perm), dtype=np.int64)
    for g in range(len(groups)):
        f, n = int(groups["first"][g]), int(groups["edges"][g])
        rg[perm[f:f + n]] = g
    return rg


def fold_groups(hist, groups, perm) -> np.ndarray:
    """[group edges][16] u64"""
    out = np.zeros((len(groups), BINS), dtype=np.uint64)
    if len(perm):
        np.add.at(out, row_group(groups, perm), np.asarray(hist[: len(perm)], dtype=np.uint64))
    return out


def fold_group_nodes(hist, groups, perm, gnodes) -> np.ndarray:
    """[workload rows][2][16] u64: the rows folded under their group refs (the group refs of a row are its group edge's)"""
    rg = row_group(groups, perm)
    return _fold_sides(hist[: len(perm)], groups["from_ref"][rg], groups["to_ref"][rg], gnodes["ref"])


def fold_group_nodes_over_groups(group_hist, groups, gnodes) -> np.ndarray:
    """the same as the sum over the group edges on each side"""
    return _fold_sides(group_hist, groups["from_ref"], groups["to_ref"], gnodes["ref"])


def node_quantiles(node_hist, nodes, permille) -> np.ndarray:
    """[n][2][n_q] u32 from a space's histograms and its rows' out_max_ns / in_max_ns"""
    mx = np.stack([nodes["out_max_ns"], nodes["in_max_ns"]], axis=1) if len(nodes) else np.zeros((0, 2), dtype=np.uint64)
    return quantiles(node_hist, mx, permille)


def group_quantiles(group_hist, groups, permille) -> np.ndarray:
    return quantiles(group_hist, groups["max_ns"], permille)
