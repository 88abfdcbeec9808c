"""numpy reference of K8's vanished list (include/servicegraph.h, "Vanished dependencies"): wraps tests/trend_ref.py's TrendRef — it
snapshots the old entries, runs the window through the baseline reference, and derives the window's vanished entries and the
alive-only row behind each one."""
import numpy as np

from alaz_amd.engine import VANISHED_DTYPE
from tests.trend_ref import TrendRef, row_keys

NO_ROW = 0xFFFFFFFF


def match_entries(old, fk, tk):
    """for each old entry the position of the row with its key, else -1 (keys are unique in both lists)"""
    B, E = len(old), len(fk)
    allf = np.concatenate([old["from_key"], fk]); allt = np.concatenate([old["to_key"], tk])
    src = np.concatenate([np.zeros(B, np.int8), np.ones(E, np.int8)])
    order = np.lexsort((src, allt, allf))
    sf, st, ss = allf[order], allt[order], src[order]
    pair = (sf[:-1] == sf[1:]) & (st[:-1] == st[1:]) & (ss[:-1] == 0) & (ss[1:] == 1)
    pos = np.flatnonzero(pair)
    m = np.full(B, -1, dtype=np.int64)
    m[order[pos]] = order[pos + 1] - B
    return m


class VanishRef:
    """window(rows, obips) -> (TREND_DTYPE rows, VANISHED_DTYPE list cut at max_rows, count of every vanished entry)"""

    def __init__(self, trend: TrendRef, silent_windows=0, min_seen=0, max_rows=0):
        self.trend = trend
        self.silent = silent_windows or 1
        self.min_seen = min_seen or trend.warmup
        self.max_rows = max_rows or min(65536, trend.cap)
        assert 1 <= self.silent < trend.ttl and self.max_rows <= trend.cap

    def window(self, rows, obips):
        old = self.trend.entries.copy()
        out = self.trend.window(rows, obips)
        w = self.trend.w
        fk, tk = row_keys(rows, obips)
        m = match_entries(old, fk, tk)
        refreshed = np.zeros(len(old), bool)
        refreshed[m >= 0] = rows["count"][m[m >= 0]] > 0
        van = ~refreshed & (old["n"] >= self.min_seen) & ((w - old["last"].astype(np.int64)) == self.silent)
        v = np.zeros(int(van.sum()), dtype=VANISHED_DTYPE)
        for f in ("from_key", "to_key", "lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last"):
            v[f] = old[f][van]
        v["row"] = np.where(m[van] >= 0, m[van], NO_ROW).astype(np.uint32)
        # a vanished entry is kept and unchanged by its window (silent < ttl, no sample)
        ent = self.trend.entries
        at = match_entries(v, ent["from_key"], ent["to_key"])
        assert (at >= 0).all()
        for f in ("lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last"):
            assert np.array_equal(ent[f][at], v[f])
        return out, v[: self.max_rows], len(v)
