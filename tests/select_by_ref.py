"""numpy references of the selection (sg_flush_window_top / sg_flush_window_top_by, include/servicegraph.h): the positions K7 selects
by a row's score, or when the key is a row's sg_edge_trend value instead."""
import numpy as np


def ref_select(rows, k, min_score):
    """positions sg_flush_window_top selects from `rows` (canonical order)"""
    s = rows["score"]
    with np.errstate(invalid="ignore"):
        ci = np.flatnonzero(s >= np.float32(min_score))
    if k == 0:
        return ci.astype(np.uint32)
    cs = s[ci].astype(np.float64) + 0.0                               # -0.0 == +0.0
    return ci[np.lexsort((ci, -cs))][:k].astype(np.uint32)


def ref_select_by(rows, trend, by, k, min_value):
    """positions selected from `rows` (canonical order) with `trend` = the window's TREND_DTYPE rows"""
    if by == "new":
        ci = np.flatnonzero((trend["windows_seen"] == 0) & (rows["count"] > 0))
        return ci[: k if k else len(ci)].astype(np.uint32)         # one key for all: canonical order
    v = trend[by]
    with np.errstate(invalid="ignore"):
        ci = np.flatnonzero(v >= np.float32(min_value))
    if k == 0:
        return ci.astype(np.uint32)
    cs = v[ci].astype(np.float64) + 0.0                               # -0.0 == +0.0
    return ci[np.lexsort((ci, -cs))][:k].astype(np.uint32)
