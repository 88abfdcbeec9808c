"""The reference of the SLO burn rates (K24; include/servicegraph.h, "SLO burn rates"): plain Python over a window's node rows or
workload rows (engine.NODE_DTYPE) and their K20 histograms ((n, 2, 16) u64, out side then in side).  Dicts by key, a deque of the
last L samples per key and side, Python integers — no ring, no running sum: every sum is taken from the deque when it is asked for.
Not a test module."""
from collections import deque

import numpy as np

from alaz_amd import engine

WORDS, ENTRY_WORDS = 18, 14
UNTRACKED = 1
SIDES = ("in", "out")                                                 # the row's side order; K20's tables hold them as (out, in)
KNOWN, LABEL, OBIP, GROUP = 0, 1, 2, 3


def budget_of(code):
    """the budget in ppm of a 12-bit budget code, None for a code that is none"""
    exp, mant = code >> 10, code & 1023
    b = mant * 10 ** exp
    return b if code < 4096 and 1 <= mant <= 1000 and b <= 999_999 else None


def objective_ok(word):
    return word == 0 or ((word >> 28) <= 14 and not (word >> 24) & 15 and budget_of(word >> 12 & 0xFFF) is not None
                         and budget_of(word & 0xFFF) is not None)


def burn_q10(bad, total, budget_ppm):
    """floor(r * 10^6 / (budget * 1024)), r = floor(min(bad, total) * 2^20 / total), 0 when total == 0"""
    if total == 0:
        return 0
    r = (min(bad, total) << 20) // total
    return r * 1_000_000 // (budget_ppm * 1024)


class SloRef:
    def __init__(self, space, mk, ml, max_groups=0, *, latency_bin, latency_target_ppm, error_target_ppm, short_windows, long_windows,
                 min_burn_q10, min_requests):
        assert space in ("nodes", "group_nodes") and 1 <= short_windows <= long_windows <= 64
        self.workload = space == "group_nodes"
        self.mk, self.ml, self.mg = mk, ml, max_groups if self.workload else 0
        self.keys = self.mg + mk + ml
        self.bin, self.lat_budget, self.err_budget = latency_bin, 1_000_000 - latency_target_ppm, 1_000_000 - error_target_ppm
        self.S, self.L, self.min_burn, self.min_requests = short_windows, long_windows, min_burn_q10, min_requests
        self.hist = {}                                                # key -> (deque of (total, err, slow) of the in side, of the out side)
        self.obj = {}                                                 # key -> objective word (absent: 0)
        self.windows = 0
        self.sides_burning = 0

    def key(self, ref):
        """the key of a ref, None for an untracked one"""
        t, v = int(ref) >> 30, int(ref) & 0x3FFFFFFF
        if t == GROUP:
            return v if self.workload and v < self.mg else None
        if t == KNOWN:
            return self.mg + v if v < self.mk else None
        if t == LABEL:
            return self.mg + self.mk + v if v < self.ml else None
        return None

    def assign(self, refs, objectives):
        ks = [self.key(r) for r in refs]
        assert all(k is not None for k in ks) and all(objective_ok(int(o)) for o in objectives)
        for k, o in zip(ks, objectives):
            self.obj[k] = int(o)

    def objective(self, key):
        """(the word, the bin, the latency budget, the error budget) key is judged by"""
        w = self.obj.get(key, 0)
        if w == 0:
            return 0, self.bin, self.lat_budget, self.err_budget
        return w, w >> 28, budget_of(w >> 12 & 0xFFF), budget_of(w & 0xFFF)

    def sums(self, key, side):
        """T_S, E_S, W_S, T_L, E_L, W_L of a key's side from its deque"""
        cols = list(zip(*self.hist[key][side]))                      # the totals, the errors, the slow counts, oldest first
        return tuple(sum(c[-self.S:]) for c in cols) + tuple(sum(c) for c in cols)

    def window(self, ents, hists):
        """close a window over its rows and their histograms: the (n, 18) u64 SLO rows"""
        out = np.zeros((len(ents), WORDS), dtype=np.uint64)
        samples = {}
        for v, e in enumerate(ents):
            key = self.key(e["ref"])
            if key is None:
                continue
            assert key not in samples, "one row per ref"
            _, b, _, _ = self.objective(key)
            two = []
            for s, side in enumerate(SIDES):
                total = int(e[f"{side}_count"])
                if total == 0:
                    two.append((0, 0, 0))
                else:
                    two.append((total, int(e[f"{side}_err"]), sum(int(x) for x in hists[v][1 - s][b + 1:])))
            samples[key] = (v, two)
        for key in set(self.hist) | set(samples):
            d = self.hist.setdefault(key, (deque(maxlen=self.L), deque(maxlen=self.L)))
            two = samples[key][1] if key in samples else ((0, 0, 0), (0, 0, 0))
            for s in range(2):
                d[s].append(two[s])
        self.windows += 1
        self.sides_burning = 0
        spans = min(self.windows, self.S) | min(self.windows, self.L) << 32
        for v, e in enumerate(ents):
            key = self.key(e["ref"])
            if key is None:
                out[v, 16] = UNTRACKED
                continue
            word, _, lat_budget, err_budget = self.objective(key)
            flags = 0
            for s in range(2):
                ts, es, ws, tl, el, wl = self.sums(key, s)
                bes, bel = burn_q10(es, ts, err_budget), burn_q10(el, tl, err_budget)
                bws, bwl = burn_q10(ws, ts, lat_budget), burn_q10(wl, tl, lat_budget)
                out[v, 8 * s: 8 * s + 8] = [ts, es, ws, tl, el, wl, bes | bel << 32, bws | bwl << 32]
                gate = tl >= self.min_requests
                f = (2 if gate and min(bes, bel) >= self.min_burn else 0) | (4 if gate and min(bws, bwl) >= self.min_burn else 0)
                flags |= f << (2 * s)
                self.sides_burning += 1 if f else 0
            out[v, 16] = flags | word << 32
            out[v, 17] = spans
        return out

    def entries(self):
        """(m, 14) u64: per key with a non-zero T_L on either side the key, the twelve sums, the objective word; ascending"""
        rows = []
        for key in sorted(self.hist):
            s = self.sums(key, 0) + self.sums(key, 1)
            if s[3] or s[9]:
                rows.append([key, *s, self.obj.get(key, 0)])
        return np.array(rows, dtype=np.uint64).reshape(len(rows), ENTRY_WORDS)

    def stats(self):
        return dict(windows=self.windows, keys_active=len(self.entries()), sides_burning=self.sides_burning, keys=max(self.keys, 1))


def slo_values(rows, by, side, min_requests):
    """a selection's value per SLO row: min(short burn, long burn) of kind `by` ("err" / "slow") on `side`, 0 for an untracked row
    or one whose T_L is below min_requests"""
    s = SIDES.index(side)
    vals = []
    for r in rows:
        b = int(r[8 * s + 6 + engine.SLOSEL_BY[by]])
        v = min(b & 0xFFFFFFFF, b >> 32)
        vals.append(0 if (int(r[16]) & UNTRACKED) or int(r[8 * s + 3]) < min_requests else v)
    return vals


def ref_select_slo(rows, by, side, k, min_value_q10, min_requests):
    """the indices sg_window_nodes_top_slo selects: the values >= min_value_q10, descending, ties by row position; the first k (k = 0:
    all of them, in row order)"""
    vals = slo_values(rows, by, side, min_requests)
    cand = [i for i, v in enumerate(vals) if v >= min_value_q10]
    if k == 0:
        return np.array(cand, dtype=np.uint32)
    cand.sort(key=lambda i: (-vals[i], i))
    return np.array(cand[:k], dtype=np.uint32)
