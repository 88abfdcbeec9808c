"""The case generator of the crafted-key selection tests (tests/select_cases.py), on the CPU: the key is monotone and invertible on
the candidates' range; the restated walk of k7_pick plus the tie rule select what the sort-based reference selects on every
generated case; and — the condition that keeps tests/test_gpu_select_keys.py from silently missing a branch — every branch of the
walk is reached on every shape that test runs, and every case whose title names a branch reaches it."""
import numpy as np
import pytest

from tests.select_by_ref import ref_select
from tests import select_cases as sc

#: every (rows, workgroups) a GPU test selects over: the edge rows and the node rows of each shape
SHAPES = sorted({(s.E, s.spans) for s in sc.EDGE_SHAPES} | {(s.N, s.node_spans) for s in sc.NODE_SHAPES})
ROWS = np.dtype([("score", "<f4")])


def _keys(c):
    return c.keys if c.keys is not None else sc.key_of(c.values, c.min_value)


def test_the_key_is_monotone_and_value_of_inverts_it():
    rng = np.random.default_rng(3)
    keys = np.unique(np.concatenate([rng.integers(sc.KEY_MIN, sc.KEY_MAX + 1, 200_000, dtype=np.uint64).astype(np.uint32),
                                     np.array([sc.KEY_MIN, sc.KEY_MIN + 1, 0x7FFFFFFE, sc.KEY_ZERO, sc.KEY_ZERO + 1, sc.KEY_MAX - 1, sc.KEY_MAX], np.uint32)]))
    keys = keys[keys != 0x7FFFFFFF]                                   # the key of no value: -0.0 has +0.0's
    v = sc.value_of(keys)
    assert not np.isnan(v).any() and (np.diff(v.astype(np.float64)) > 0).all()             # ascending keys, ascending values
    assert np.array_equal(sc.key_of(v), keys)
    assert v[0] == -np.inf and v[-1] == np.inf
    assert sc.key_of(-0.0)[0] == sc.key_of(0.0)[0] == sc.KEY_ZERO and sc.value_of(0x7FFFFFFF).view(np.uint32)[0] == 0x80000000
    # outside the range: NaNs, never candidates
    out = np.array([1, 0xFF, sc.KEY_MIN - 1, sc.KEY_MAX + 1, 0xFFFFFFFF], np.uint32)
    assert np.isnan(sc.value_of(out)).all() and not sc.key_of(sc.value_of(out)).any()
    # values, the other way round: sorted values have sorted keys, equal only for the two zeros
    x = np.sort(np.concatenate([sc.bits(rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)), sc.bits(sc.SPECIALS)]))
    x = x[~np.isnan(x)]
    kx = sc.key_of(x).astype(np.int64)
    assert (np.diff(kx) >= 0).all() and ((np.diff(kx) == 0) == (np.diff(x.astype(np.float64)) == 0)).all()
    assert sc.key_of(x, 0.0)[x < 0].sum() == 0 and (sc.key_of(x, 0.0)[x >= 0] != 0).all()
    assert not sc.key_of(x, sc.NAN).any()


@pytest.mark.parametrize("E,spans", SHAPES)
def test_walk_and_tie_rule_select_what_the_reference_selects(E, spans):
    n = 0
    for c in sc.cases(E, spans):
        keys = _keys(c)
        got = sc.compact(keys, c.k)
        if c.keys is None:
            rows = np.zeros(E, ROWS); rows["score"] = c.values
            want = ref_select(rows, c.k, c.min_value)
        else:                                                         # raw keys: their own sort
            pos = np.flatnonzero(keys)
            want = pos[np.lexsort((pos, -keys[pos].astype(np.int64)))][: c.k]
            assert np.isnan(c.values).all()                           # ... and on the device none of them is a candidate
        assert np.array_equal(got, want), c.name
        n += 1
    assert n > 40 or E < 2


@pytest.mark.parametrize("E,spans", SHAPES)
def test_every_branch_is_reached_on_every_shape(E, spans):
    reached, names = set(), set()
    for c in sc.cases(E, spans):
        assert c.name not in names, c.name
        names.add(c.name)
        if c.k == 0:
            assert c.expect is None
            continue
        w = sc.walk(_keys(c), c.k)
        assert not w.p_zero, c.name                                   # (select_cases' docstring: never reached)
        if c.expect is not None:
            assert w.branch == c.expect, (c.name, w)
        if c.keys is None:
            reached.add(w.branch)
    # one row: k >= 1 takes it, nothing else can happen
    assert reached == (set(sc.BRANCHES) if E >= 2 else {"all_fit"}), sorted(set(sc.BRANCHES) - reached)
    per_family = {f: {sc.walk(_keys(c), c.k).branch for c in sc.cases(E, spans, (f,)) if c.k and c.keys is None} for f in ("ties", "specials")}
    assert E < 2 or "ties@3" in per_family["ties"]                    # the families every shape of every space runs


def test_the_tie_cases_end_where_their_titles_say():
    """the last tie taken against the span and the tile it is named after (spans of ceil(E / spans) rows, tiles of 256 from a span's start)"""
    for E, spans in SHAPES:
        if E < 2:
            continue
        L = -(-E // spans)
        seen = set()
        for c in sc.cases(E, spans, ("ties",)):
            keys = sc.key_of(c.values)
            w = sc.walk(keys, c.k)
            if w.branch != "ties@3":
                continue
            last = int(np.flatnonzero(keys == w.T)[w.need - 1])       # the row of the last tie taken
            nxt = np.flatnonzero(keys == w.T)[w.need:]
            if "inside the first span" in c.name:
                assert last < L and nxt[0] < L; seen.add("first")
            if "at the end of the first span" in c.name:
                assert last < L <= nxt[0]; seen.add("end")
            if "inside the last span" in c.name:
                assert last >= ((E - 1) // L) * L; seen.add("last")
            if "last row of a tile" in c.name:
                lo = int(c.name.rsplit(" ", 1)[1])
                assert last == lo + sc.TILE - 1 and nxt[0] == lo + sc.TILE; seen.add("tile-")
            if "first row of the next tile" in c.name:
                lo = int(c.name.rsplit(" ", 1)[1])
                assert last == lo + sc.TILE and nxt[0] == lo + sc.TILE + 1; seen.add("tile+")
            if "-0.0 and +0.0" in c.name:
                z = c.values[keys == w.T].view(np.uint32)
                assert w.T == sc.KEY_ZERO and {0, 0x80000000} <= set(z.tolist()); seen.add("zeros")
        assert "zeros" in seen or E < 3, (E, spans, seen)
        assert L < 2 or "first" in seen, (E, spans, seen)
        assert E - 2 < ((E - 1) // L) * L or "last" in seen, (E, spans, seen)
        assert (L <= sc.TILE + 6) or {"tile-", "tile+"} <= seen, (E, spans, seen)
        assert spans == 1 or E <= L or "end" in seen, (E, spans, seen)


def test_the_specials_and_counts_hold_what_they_name():
    E = 2049
    sp = list(sc.cases(E, 2, ("specials",)))
    assert set(sc.SPECIALS.tolist()) <= set(sp[0].values.view(np.uint32).tolist())
    mvs = {repr(np.float32(c.min_value)) for c in sp}
    assert len(mvs) == 7 and any(np.isnan(c.min_value) for c in sp)
    assert any(np.float32(c.min_value).view(np.uint32) == 0x80000000 for c in sp)      # -0.0 as the threshold
    ks = {c.k for c in sc.cases(20_000, 16, ("counts",))}
    assert {0, 1, 2, 3, 255, 256, 257, 1000, 16383, 16384} <= ks
    full = [c for c in sc.cases(20_000, 16, ("counts",)) if c.k == 16384 and int((sc.key_of(c.values, c.min_value) != 0).sum()) >= 16384]
    assert len(full) == 2                                             # k = m = n = 16 384 and one candidate more: the sort with no pad
    pad = [c for c in sc.cases(2049, 2, ("counts",)) if c.k == 1000 and int((sc.key_of(c.values, c.min_value) != 0).sum()) >= 1000]
    assert len(pad) == 2                                              # 1 000 selected: sorted in 1 024 slots with 24 pads
