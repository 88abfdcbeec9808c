"""Crafted inputs for K7, the selection (alaz_amd/csrc/sg_sel.h): plain numpy, no GPU.

key_of / value_of restate k7_key; walk restates the four rounds of k7_pick and names the branch that decided; compact restates the
tie rule of k7_scatter / k7_sort.  cases(E, spans) yields named (values, k, min_value) triples that aim at each branch and at the
places the parallel passes can slip: the per-workgroup spans of k7_span (span length ceil(E / spans)), the 256-row tiles of
k7_scatter, the sort's padding, the values a score never takes.  walk and compact classify the cases (tests/test_select_cases.py);
no expected value of a GPU test comes from them — those come from the sort-based references of tests/select_by_ref.py.

Keys.  A candidate's key is its float's bits made order-preserving: a negative float's bits inverted, else the sign bit set; -0.0
takes +0.0's key 0x80000000, so 0x7FFFFFFF is the key of no value.  Candidates' keys lie in [0x007FFFFF, 0xFF800000] (-inf .. +inf);
what lies outside decodes to a NaN, which is never a candidate; 0 is the key of every row that is no candidate.

The `p ? p - 1 : 0` arm of k7_pick.  A whole bin at round r with p == 0 is the lowest bin of a round whose higher bytes are all 0.
The lowest bin ending at rem exactly means every key of the round's prefix is taken, so the bin picked at round r - 1 ended at its
rem exactly too and the walk stopped there; at round 0 that is `all candidates fit`, which is tested first.  So p == 0 is never
reached, whatever the keys: walk reports it (Walk.p_zero), and tests/test_select_cases.py holds it False on every case, the raw-key
ladder 0x000000xx included."""
from collections import namedtuple

import numpy as np

KEY_MIN, KEY_MAX = 0x007FFFFF, 0xFF800000         # the keys of -inf and +inf
KEY_ZERO = 0x80000000                             # of -0.0 and +0.0
TILE = 256                                        # rows per k7_scatter tile (K7_THREADS)
MAX_K = 16384                                     # SG_SELECT_MAX_K
NEG_INF, INF, NAN = float("-inf"), float("inf"), float("nan")
FLT_MAX = float(np.finfo(np.float32).max)

Case = namedtuple("Case", "name values k min_value expect keys")
Case.__doc__ = """values [E] float32, k (0 = threshold mode), min_value; expect: the branch of walk the title names (or None); keys: raw
keys for walk alone where the case is about keys no value has (else None: key_of(values, min_value))"""
Walk = namedtuple("Walk", "branch T need p_zero")
Shape = namedtuple("Shape", "max_edges fed E spans max_known N node_spans")
Shape.__doc__ = """a window the GPU test closes: an engine of max_edges (and max_known nodes, None = the topology's) fed `fed` distinct edges of
tests/test_gpu_pair_tiles' topology has E rows over `spans` workgroups and N node rows over node_spans (None: not used by node tests)"""
BRANCHES = ("all_fit", "whole_bin@0", "whole_bin@1", "whole_bin@2", "whole_bin@3", "ties@3")


def _f32(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float32))


def bits(u):
    """float32 values of u32 bit patterns"""
    return np.atleast_1d(np.asarray(u, dtype=np.uint32)).view(np.float32)


def key_of(value, min_value=NEG_INF):
    """k7_key: the order-preserving u32 key of each value, 0 where it is no candidate (not value >= min_value)"""
    v = _f32(value)
    u = v.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        cand = v >= np.float32(min_value)
    return np.where(cand, key, np.uint32(0)).astype(np.uint32)


def value_of(key):
    """the value of a key (+0.0 for KEY_ZERO); a key outside [KEY_MIN, KEY_MAX] gives a NaN"""
    k = np.atleast_1d(np.asarray(key, dtype=np.uint32))
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def walk(keys, k):
    """the four rounds of k7_pick over `keys` (0 = no candidate), k > 0: Walk(branch, T, need, p_zero) — select the keys > T and the
    first `need` rows with key == T"""
    assert k > 0
    keys = np.asarray(keys, dtype=np.uint32)
    keys = keys[keys != 0].astype(np.uint64)
    prefix, rem = 0, int(k)
    for r in range(4):
        shift = 24 - 8 * r
        hmask = (0xFFFFFFFF << (32 - 8 * r)) & 0xFFFFFFFF
        live = keys[(keys & np.uint64(hmask)) == np.uint64(prefix)]
        hist = np.bincount(((live >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        if r == 0 and int(hist.sum()) <= rem:
            return Walk("all_fit", 0, 0, False)
        above = 0
        for d in range(255, -1, -1):
            c = int(hist[d])
            if above < rem <= above + c:
                p = prefix | (d << shift)
                if above + c == rem:
                    return Walk(f"whole_bin@{r}", p - 1 if p else 0, 0, p == 0)
                prefix, rem = p, rem - above
                break
            above += c
        else:
            raise AssertionError("no bin holds the k-th key")
    return Walk("ties@3", prefix, rem, False)


def compact(keys, k, w=None):
    """positions selected from `keys` by the tie rule: threshold mode (k = 0) every key > 0 in row order; top-k the keys > T and the
    first `need` keys == T, ordered by key descending, then row"""
    keys = np.asarray(keys, dtype=np.uint32)
    if k == 0:
        return np.flatnonzero(keys).astype(np.uint32)
    w = w or walk(keys, k)
    gt, eq = keys > np.uint32(w.T), keys == np.uint32(w.T)
    eq_before = np.cumsum(eq) - eq
    pos = np.flatnonzero(gt | (eq & (eq_before < w.need)))
    return pos[np.lexsort((pos, -keys[pos].astype(np.int64)))].astype(np.uint32)


# ---- the families ---------------------------------------------------------------------------------------------------------------------
def _span_len(E, spans):
    return -(-E // spans) if E else 0


def _ladder(E, r, prefix, steps, rng):
    """E keys sharing their top r bytes (`prefix`, r bytes), byte r one of the three `steps` (descending) with counts of about a
    quarter, a third and the rest, the lower bytes random; shuffled over the rows.  -> (keys, count of the top bin, of the second)"""
    n_hi = max(1, E // 4)
    n_mid = max(1, E // 3) if E >= 3 else 0
    n_lo = E - n_hi - n_mid
    shift = 24 - 8 * r
    byte = np.repeat(np.array(steps, dtype=np.uint64), [n_hi, n_mid, n_lo])
    low = rng.integers(0, 1 << shift, E, dtype=np.uint64) if shift else np.zeros(E, np.uint64)
    keys = ((np.uint64(prefix) << np.uint64(shift + 8)) | (byte << np.uint64(shift)) | low).astype(np.uint32)
    return keys[rng.permutation(E)], n_hi, n_mid, n_lo


#: (title, round, the r shared top bytes, the three values of byte r): values near 1 (a sigmoid's range), negative values, the
#: lowest and the highest finite keys (beside the NaN ranges)
LADDERS = [("r0", 0, 0x0, (0xC1, 0xBF, 0x3E)),
           ("r1", 1, 0xBF, (0xE0, 0x80, 0x01)),
           ("r2", 2, 0xBF40, (0xFF, 0x7F, 0x00)),
           ("r3", 3, 0xBF4000, (0xFF, 0x80, 0x00)),
           ("r1 negative", 1, 0x40, (0xC0, 0x7F, 0x10)),
           ("r3 negative", 3, 0x40C000, (0x03, 0x02, 0x01)),
           ("r3 lowest finite", 3, 0x008000, (0x02, 0x01, 0x00)),
           ("r3 highest finite", 3, 0xFF7FFF, (0xFF, 0xFE, 0xFD))]


def _ladders(E, rng):
    if E < 2:
        return
    for title, r, prefix, steps in LADDERS:
        keys, n_hi, n_mid, n_lo = _ladder(E, r, prefix, steps, rng)
        assert KEY_MIN <= int(keys.min()) and int(keys.max()) <= KEY_MAX
        v = value_of(keys)
        if n_hi <= MAX_K:
            yield Case(f"ladder {title}: k ends the top bin", v, n_hi, NEG_INF, f"whole_bin@{r}", None)
        if n_lo and n_hi + n_mid <= MAX_K:
            yield Case(f"ladder {title}: k ends the second bin", v, n_hi + n_mid, NEG_INF, f"whole_bin@{r}", None)
        if n_mid >= 2 and n_hi + n_mid // 2 <= MAX_K:
            yield Case(f"ladder {title}: k inside the second bin", v, n_hi + n_mid // 2, NEG_INF, "ties@3" if r == 3 else None, None)
    # keys 0x000000xx: bits no candidate has (they decode to negative NaNs) — the device selects nothing; walk takes them raw
    keys, n_hi, n_mid, n_lo = _ladder(E, 3, 0x000000, (0x03, 0x02, 0x01), rng)
    for what, k in (("top", n_hi), ("second", n_hi + n_mid)):
        if k <= MAX_K and k < E:
            yield Case(f"ladder zero prefix (NaN bits): k ends the {what} bin", value_of(keys), k, NEG_INF, "whole_bin@3", keys)


def _tie_case(name, E, tie, need, rng, T=1.25, share_above=0.4):
    """rows `tie` (a mask) hold T, about share_above of the others a larger value, the rest a smaller one; k = the larger ones + need"""
    v = np.where(rng.random(E) < share_above, np.float32(T) + rng.integers(1, 1 << 20, E).astype(np.float32), np.float32(T) - rng.integers(1, 1 << 20, E).astype(np.float32))
    v = v.astype(np.float32)
    v[tie] = T
    k = int((v > np.float32(T)).sum()) + need
    if not 0 < k <= MAX_K:
        return None
    return Case(name, v, k, NEG_INF, "ties@3" if 0 < need < int(tie.sum()) else None, None)


def _ties(E, spans, rng):
    if E < 2:
        return
    L = _span_len(E, spans)
    tie = rng.random(E) < 0.4
    tie[[0, 1, E - 2, E - 1]] = True                                  # two ties in the first span and two in the last
    nt, first = int(tie.sum()), int(tie[:L].sum())
    last_lo = ((E - 1) // L) * L                                      # the last span that has rows
    out = [_tie_case("ties: run out at the end of the first span", E, tie, first, rng),
           _tie_case("ties: every tie but none to spare", E, tie, nt, rng)]
    if first >= 2:
        out.append(_tie_case("ties: run out inside the first span", E, tie, 1, rng))
    if E - 2 >= last_lo:
        out.append(_tie_case("ties: run out inside the last span", E, tie, nt - 1, rng))
    if last_lo:
        out.append(_tie_case("ties: run out at the start of the last span", E, tie, int(tie[:last_lo].sum()) + 1, rng))
        out.append(_tie_case("ties: run out at the end of the span before the last", E, tie, int(tie[:last_lo].sum()), rng))
    for lo in sorted({0, last_lo}):                                   # the 256-row tiles of a span: the last row of one, the first of the next
        if min(lo + L, E) - lo > TILE + 6:
            t = rng.random(E) < 0.05
            t[lo + TILE - 6:lo + TILE + 6] = True
            for at, what in ((lo + TILE - 1, "on the last row of a tile"), (lo + TILE, "on the first row of the next tile")):
                out.append(_tie_case(f"ties: the last one taken {what} of the span at {lo}", E, t, int(t[:at + 1].sum()), rng))
    z = rng.random(E) < 0.5                                           # -0.0 and +0.0: one key, ordered by position
    z[[0, E - 1]] = True
    c = _tie_case("ties: -0.0 and +0.0 mixed", E, z, max(1, int(z.sum()) // 2), rng, T=0.0)
    if c is not None:
        v = c.values.copy()
        v[np.flatnonzero(z)[::2]] = -0.0
        out.append(c._replace(values=v))
    for k in sorted({1, E // 2, E - 1} - {0}):
        if k <= MAX_K:
            out.append(Case(f"ties: all rows equal, k = {k}", np.full(E, 0.75, np.float32), k, NEG_INF, "ties@3", None))
    yield from (c for c in out if c is not None)


#: ±0, ±inf, NaNs of both signs with and without payload, the smallest denormals, ±FLT_MAX, negative and ordinary values
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
                     0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0xBFC00000, 0x3FC00000, 0x3FC00001, 0x3E800000, 0xC2F60000],
                    dtype=np.uint32)
PRESENT = 1.5                                                         # 0x3FC00000, a value of SPECIALS


def _specials(E, rng):
    if E == 0:
        return
    v = bits(SPECIALS[rng.integers(0, len(SPECIALS), E)])
    v[: min(E, len(SPECIALS))] = bits(SPECIALS)[rng.permutation(len(SPECIALS))[: min(E, len(SPECIALS))]]
    above = float(np.nextafter(np.float32(PRESENT), np.float32(np.inf)))
    for mv, title in ((NEG_INF, "-inf"), (INF, "+inf"), (-0.0, "-0.0"), (0.0, "0.0"), (NAN, "NaN"), (PRESENT, "a value present"), (above, "the next value above it")):
        for k in sorted({0, 1, 3, (E + 1) // 2, E + 1}):
            if k <= MAX_K:
                yield Case(f"specials: min_value {title}, k = {k}", v, k, mv, None, None)


def _counts(E, rng):
    v = rng.permutation(E).astype(np.float32) / np.float32(max(E, 1))   # E distinct values of [0, 1)
    desc = np.sort(v)[::-1]
    for c in sorted({0, E // 2, E}):
        yield Case(f"counts: threshold mode, {c} candidates", v, 0, INF if c == 0 else float(desc[c - 1]), None, None)
    for k in (1, 2, 3, 255, 256, 257, 1000, 16383, 16384):
        for c in sorted({0, k - 1, k, k + 1}):
            if c <= E:
                mv = INF if c == 0 else float(desc[c - 1])
                yield Case(f"counts: k = {k}, {c} candidates", v, k, mv, "all_fit" if c <= k else None, None)
        if k > E:
            yield Case(f"counts: k = {k} beyond the {E} rows", v, k, NEG_INF, "all_fit", None)


def _random_bits(E, rng):
    for s in range(3):
        v = bits(rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(np.uint32))
        for k in sorted({0, 1, E // 3, min(E, 1000)}):
            yield Case(f"random bits {s}: k = {k}", v, k, (NEG_INF, 0.0, -1e30)[s], None, None)


#: engine A, 4 096 edges (2 workgroups; 3 584 node keys: 2): windows of 1, 2, 3 rows, 257, 2 049 (a span of 1 025: one trip of
#: k7_keys' unrolled body and its tail), and the keys array full, from more distinct edges than fit (which of them stay, and so the
#: node rows, differs from run to run).  Engine B, 32 768 edges (16 workgroups) and as many known nodes (33 344 node keys: 17):
#: 20 rows (six workgroups with empty spans; 22 node rows: six of 17) and 20 000 (k = 16 384 with as many candidates: the full sort)
EDGE_SHAPES = tuple([Shape(4096, n, n, 2, None, N, 2) for n, N in ((1, 2), (2, 3), (3, 4), (257, 219), (2049, 1026))]
                    + [Shape(4096, 6000, 4096, 2, None, None, 2), Shape(1 << 15, 20, 20, 16, 1 << 15, 22, 17),
                       Shape(1 << 15, 20_000, 20_000, 16, 1 << 15, 2646, 17)])
NODE_SHAPES = tuple(s for s in EDGE_SHAPES if s.N is not None)

FAMILIES = ("ladders", "ties", "specials", "counts", "random")


def cases(E, spans, families=FAMILIES, seed=7):
    """the named cases for a window of E rows selected by `spans` workgroups"""
    rng = np.random.default_rng([seed, E, spans])
    gen = dict(ladders=lambda: _ladders(E, rng), ties=lambda: _ties(E, spans, rng), specials=lambda: _specials(E, rng),
               counts=lambda: _counts(E, rng), random=lambda: _random_bits(E, rng))
    for f in FAMILIES:
        if f in families:
            for c in gen[f]():
                assert c.values.dtype == np.float32 and len(c.values) == E and 0 <= c.k <= MAX_K, c.name
                yield c


def new_masks(E, spans, seed=11):
    """for the keys that are one key for every flagged row (SG_SEL_NEW / SG_NSEL_NEW: all ties, by position): named (mask [E] bool, k)"""
    rng = np.random.default_rng([seed, E, spans])
    L = _span_len(E, spans)
    for title, m in (("none", np.zeros(E, bool)), ("all", np.ones(E, bool)), ("half", rng.random(E) < 0.5), ("few", rng.random(E) < 0.03)):
        n = int(m.sum())
        first = int(m[:L].sum())
        for k in sorted({0, 1, first, first + 1, n - 1, n, n + 1, min(int(m[:L + TILE].sum()), n)} - {-1}):
            if k <= MAX_K:
                yield f"new: {title} flagged, k = {k}", m, k
