"""CPU tests of the SLO burn rates (K24): the reference of tests/slo_ref.py against a second formulation written apart from it (the
full list of past windows, every sum recomputed from it, no deque), against hand-computed answers, the plan in
alaz_amd/csrc/sg_plan.hpp (tests/micro/slo_plan_test.cpp against tests/golden/slo_plan.json) and the header's constants against
alaz_amd/engine.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.engine import NODE_DTYPE
from tests.helpers import G
from tests.slo_ref import SloRef, burn_q10, objective_ok, ref_select_slo, slo_values

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LABEL, OBIP = 1 << 30, 2 << 30
P = dict(latency_bin=3, latency_target_ppm=990_000, error_target_ppm=999_000, short_windows=2, long_windows=4, min_burn_q10=1024, min_requests=10)


def _ents(rows):
    """node rows from (ref, in_count, in_err, out_count, out_err)"""
    e = np.zeros(len(rows), dtype=NODE_DTYPE)
    for k, (ref, ic, ie, oc, oe) in enumerate(rows):
        e[k]["ref"], e[k]["in_count"], e[k]["in_err"], e[k]["out_count"], e[k]["out_err"] = ref, ic, ie, oc, oe
    return e


def _hist(ents, in_bins=None, out_bins=None):
    """(n, 2, 16) u64, out side then in side: every request in bin 0 unless {row: {bin: count}} says otherwise"""
    h = np.zeros((len(ents), 2, 16), dtype=np.uint64)
    for side, name, over in ((0, "out_count", out_bins or {}), (1, "in_count", in_bins or {})):
        for k in range(len(ents)):
            bins = over.get(k, {})
            for b, c in bins.items():
                h[k, side, b] = c
            h[k, side, 0] = int(ents[k][name]) - sum(bins.values())
    return h


def _close(ref, rows, **bins):
    e = _ents(rows)
    return ref.window(e, _hist(e, **bins))


# ---- 1. a second formulation ---------------------------------------------------------------------------------------------------------
class Plain:
    """every window's samples kept for ever; a sum is taken over the last S or L of ALL windows, a key without a sample counting zero"""

    def __init__(self, workload, mk, ml, mg, p):
        self.workload, self.mk, self.ml, self.mg, self.p = workload, mk, ml, mg if workload else 0, p
        self.past, self.words = [], {}

    def key(self, ref):
        kind, v = ref >> 30, ref & ((1 << 30) - 1)
        if kind == 3 and self.workload and v < self.mg:
            return v
        if kind == 0 and v < self.mk:
            return self.mg + v
        if kind == 1 and v < self.ml:
            return self.mg + self.mk + v
        return -1

    def judged(self, key):
        w = self.words.get(key, 0)
        if not w:
            return 0, self.p["latency_bin"], 10 ** 6 - self.p["latency_target_ppm"], 10 ** 6 - self.p["error_target_ppm"]
        code = lambda c: (c % 1024) * (1, 10, 100, 1000)[c // 1024]
        return w, w // 2 ** 28, code(w // 4096 % 4096), code(w % 4096)

    def window(self, ents, hist):
        now = {}
        for v in range(len(ents)):
            key = self.key(int(ents["ref"][v]))
            if key < 0:
                continue
            b = self.judged(key)[1]
            for s, (cnt, err, hs) in enumerate((("in_count", "in_err", 1), ("out_count", "out_err", 0))):
                t = int(ents[cnt][v])
                now[key, s] = (t, int(ents[err][v]), int(hist[v, hs, b + 1:].astype(object).sum())) if t else (0, 0, 0)
        self.past.append(now)
        out = []
        for v in range(len(ents)):
            key = self.key(int(ents["ref"][v]))
            if key < 0:
                out.append([0] * 16 + [1, 0])
                continue
            word, _, lb, eb = self.judged(key)
            row, flags = [], 0
            for s in range(2):
                tot = []
                for span in (self.p["short_windows"], self.p["long_windows"]):
                    tot += [sum(w.get((key, s), (0, 0, 0))[j] for w in self.past[-span:]) for j in range(3)]
                ratio = lambda bad, total: 0 if not total else (min(bad, total) * 2 ** 20 // total) * 10 ** 6
                be = [ratio(tot[1], tot[0]) // (eb * 1024), ratio(tot[4], tot[3]) // (eb * 1024)]
                bw = [ratio(tot[2], tot[0]) // (lb * 1024), ratio(tot[5], tot[3]) // (lb * 1024)]
                row += tot + [be[0] + be[1] * 2 ** 32, bw[0] + bw[1] * 2 ** 32]
                if tot[3] >= self.p["min_requests"]:
                    flags += (2 if min(be) >= self.p["min_burn_q10"] else 0) * 4 ** s + (4 if min(bw) >= self.p["min_burn_q10"] else 0) * 4 ** s
            n = len(self.past)
            out.append(row + [flags + word * 2 ** 32, min(n, self.p["short_windows"]) + min(n, self.p["long_windows"]) * 2 ** 32])
        return np.array(out, dtype=np.uint64).reshape(len(ents), 18)


def _random_window(rng, refs, mk):
    pick = refs[rng.random(len(refs)) < rng.uniform(0.2, 0.9)]
    e = np.zeros(len(pick), dtype=NODE_DTYPE)
    e["ref"] = pick
    for side in ("in", "out"):
        c = rng.integers(0, 40, len(pick)) * (rng.random(len(pick)) < 0.8)
        e[f"{side}_count"] = c
        e[f"{side}_err"] = (c * rng.random(len(pick)) * (rng.random(len(pick)) < 0.5)).astype(np.uint64)
    h = np.zeros((len(pick), 2, 16), dtype=np.uint64)
    for k in range(len(pick)):
        for hs, side in ((0, "out"), (1, "in")):
            h[k, hs] = np.bincount(rng.integers(0, 16, int(e[f"{side}_count"][k])), minlength=16)
    return e, h


def test_the_reference_is_the_plain_formulation_over_300_random_chains():
    rng = np.random.default_rng(24)
    mk, ml, mg = 12, 4, 5
    pool = {False: np.array(list(range(mk)) + [LABEL | v for v in range(ml)] + [OBIP | v for v in range(3)], dtype=np.uint32),
            True: np.array([G(v) for v in range(mg)] + list(range(mk)) + [LABEL | v for v in range(ml)] + [OBIP | v for v in range(3)], dtype=np.uint32)}
    spans = (1, 2, 3, 5, 64)
    for chain in range(300):
        workload = bool(chain & 1)
        S, L = sorted(rng.choice(spans, 2))
        p = dict(latency_bin=int(rng.integers(0, 15)), latency_target_ppm=int(rng.choice([500_000, 990_000, 999_999])),
                 error_target_ppm=int(rng.choice([1, 900_000, 999_900])), short_windows=int(S), long_windows=int(L),
                 min_burn_q10=int(rng.choice([0, 1024, 14746])), min_requests=int(rng.choice([0, 1, 50])))
        ref = SloRef("group_nodes" if workload else "nodes", mk, ml, mg, **p)
        plain = Plain(workload, mk, ml, mg, p)
        refs = pool[workload]
        for w in range(int(rng.integers(6, 13))):
            if rng.random() < 0.3:                                    # an objective for a key, or its reset, between windows
                r = int(rng.choice(refs[refs >> 30 != 2]))
                word = 0 if rng.random() < 0.3 else engine.slo_objective(int(rng.integers(0, 15)), 999_000, int(rng.choice([990_000, 999_999])))
                ref.assign([r], [word]); plain.words[plain.key(r)] = word
            e, h = _random_window(rng, refs, mk)
            got, want = ref.window(e, h), plain.window(e, h)
            assert got.tobytes() == want.tobytes(), (chain, w, p)
        ent = ref.entries()
        live = sorted({k for k, s in plain.past[-1].keys()} | {k for w in plain.past[-L:] for (k, s), x in w.items() if x[0]})
        assert ent[:, 0].tolist() == [k for k in live if any(w.get((k, s), (0,))[0] for w in plain.past[-L:] for s in (0, 1))]
        assert ref.stats()["windows"] == len(plain.past) and ref.stats()["keys_active"] == len(ent)


# ---- 2. hand-computed answers ----------------------------------------------------------------------------------------------------------
def test_the_burn_rate_by_hand():
    assert burn_q10(0, 0, 1000) == 0 and burn_q10(5, 0, 1000) == 0                       # total == 0
    assert burn_q10(3, 1000, 1000) == 3071                            # r = floor(3145.728) = 3145; 3145 * 10^6 / 1 024 000 = 3071.28
    assert burn_q10(1, 3, 10_000) == 34133                            # r = 349525; / 10.24 = 34133.3
    assert burn_q10(7, 7, 1) == 1_024_000_000 < 2 ** 32               # budget 1 ppm, every request bad: the largest burn
    assert burn_q10(9, 7, 1) == 1_024_000_000                         # bad is capped at total
    assert burn_q10(2 ** 40 // 3, 2 ** 40, 10_000) == 34133 and burn_q10(1, 2 ** 40, 1) == 0
    assert burn_q10(2 ** 63, 2 ** 63, 1) == 1_024_000_000 and burn_q10(2 ** 63 - 1, 2 ** 63, 1000) == 1_023_999
    assert burn_q10(2 ** 62, 2 ** 63, 1000) == 512_000               # exactly half: r = 2^19


def test_counts_of_two_to_the_forty_and_sixty_three_through_the_rows():
    ref = SloRef("nodes", 8, 2, **{**P, "short_windows": 1, "long_windows": 1})
    r = _close(ref, [(1, 2 ** 63, 2 ** 63 - 1, 2 ** 40, 2 ** 40 // 3)], in_bins={0: {9: 2 ** 62}}, out_bins={0: {4: 1}})[0]
    assert r[:6].tolist() == [2 ** 63, 2 ** 63 - 1, 2 ** 62, 2 ** 63, 2 ** 63 - 1, 2 ** 62]
    assert int(r[6]) == 1_023_999 * (1 + 2 ** 32) and int(r[7]) == 51_200 * (1 + 2 ** 32)      # budgets 1000 and 10 000 ppm
    assert r[8:14].tolist() == [2 ** 40, 2 ** 40 // 3, 1] * 2 and int(r[14]) == 341_333 * (1 + 2 ** 32) and int(r[15]) == 0
    assert int(r[16]) == 2 | 4 | 8 and int(r[17]) == 1 | 1 << 32


def test_warm_up_then_full_spans_and_a_burst_that_leaves_the_short_span_first():
    ref = SloRef("nodes", 8, 2, **P)                                  # S = 2, L = 4
    rows = [_close(ref, [(5, 100, 50 if w == 0 else 0, 0, 0)])[0] for w in range(6)]
    assert [int(r[17]) for r in rows] == [1 | 1 << 32, 2 | 2 << 32, 2 | 3 << 32, 2 | 4 << 32, 2 | 4 << 32, 2 | 4 << 32]
    assert [r[:6].tolist() for r in rows] == [[100, 50, 0, 100, 50, 0], [200, 50, 0, 200, 50, 0], [200, 0, 0, 300, 50, 0],
                                              [200, 0, 0, 400, 50, 0], [200, 0, 0, 400, 0, 0], [200, 0, 0, 400, 0, 0]]
    # budget 1000 ppm: half bad = 512 000, a quarter 256 000, a sixth 170 666, an eighth 128 000
    assert [(int(r[6]) & 0xFFFFFFFF, int(r[6]) >> 32) for r in rows[:4]] == [(512_000, 512_000), (256_000, 256_000), (0, 170_666), (0, 128_000)]
    assert [int(r[16]) for r in rows] == [2, 2, 0, 0, 0, 0]          # burning needs BOTH spans over the threshold
    assert all((r[8:16] == 0).all() for r in rows)                    # the out side: count 0 samples zeros


@pytest.mark.parametrize("S,L", [(1, 1), (3, 3), (1, 3)])
def test_equal_spans_and_a_span_of_one(S, L):
    ref = SloRef("nodes", 8, 2, **{**P, "short_windows": S, "long_windows": L})
    tot = []
    for w in range(7):
        r = _close(ref, [(2, 10 + w, w, 0, 0)])[0]
        tot.append((int(r[0]), int(r[1]), int(r[3]), int(r[4])))
    want = []
    for w in range(7):
        s, l = range(max(0, w - S + 1), w + 1), range(max(0, w - L + 1), w + 1)
        want.append((sum(10 + x for x in s), sum(s), sum(10 + x for x in l), sum(l)))
    assert tot == want
    if S == L:
        assert all(t[:2] == t[2:] for t in tot)


@pytest.mark.parametrize("gap", [3, 4, 5])
def test_a_key_silent_for_l_minus_one_l_and_l_plus_one_windows(gap):
    """L = 4: after L - 1 silent windows the last sample is still in the long span, after L or more nothing is, and the entry is gone"""
    ref = SloRef("nodes", 8, 2, **P)
    _close(ref, [(3, 40, 4, 0, 0), (4, 1, 0, 1, 0)])
    for _ in range(gap):
        _close(ref, [(4, 1, 0, 1, 0)])
        keys = ref.entries()[:, 0].tolist()
    assert (3 in keys) == (gap < 4) and 4 in keys
    r = _close(ref, [(3, 7, 7, 0, 0), (4, 1, 0, 1, 0)])[0]
    assert r[:6].tolist() == [7, 7, 0, 7, 7, 0]                       # the window of the return is the L-th after it at the least: it left
    ref = SloRef("nodes", 8, 2, **P)
    _close(ref, [(3, 40, 4, 0, 0)])
    for _ in range(2):
        _close(ref, [])
    assert _close(ref, [(3, 7, 7, 0, 0)])[0][:6].tolist() == [7, 7, 0, 47, 11, 0]     # two silent windows: still inside


def test_the_min_requests_gate_on_either_side_of_its_value():
    for total, flag in ((9, 0), (10, 2), (11, 2)):
        ref = SloRef("nodes", 8, 2, **P)                              # min_requests 10
        r = _close(ref, [(1, total, total, 0, 0)])[0]
        assert int(r[16]) == flag and int(r[6]) == 1_024_000 * (1 + 2 ** 32)     # the burn itself is reported either way
        rows = np.array([r])
        assert slo_values(rows, "err", "in", 10) == [1_024_000 if flag else 0]
        assert ref_select_slo(rows, "err", "in", 1, 1, 10).tolist() == ([0] if flag else [])
    ref = SloRef("nodes", 8, 2, **P)
    a = _close(ref, [(1, 9, 9, 0, 0)])[0]
    b = _close(ref, [(1, 1, 1, 0, 0)])[0]                             # the gate is on T_L, the long span's total
    assert (int(a[16]), int(b[16]), int(b[3])) == (0, 2, 10)


def test_the_slow_count_is_the_bins_above_the_objectives_bin_and_sides_map_to_k20s():
    ref = SloRef("nodes", 8, 2, **P)                                  # latency_bin 3, budget 10 000 ppm
    r = _close(ref, [(6, 100, 0, 50, 0)], in_bins={0: {3: 60, 4: 30, 15: 10}}, out_bins={0: {2: 49, 14: 1}})[0]
    assert int(r[2]) == 40 and int(r[10]) == 1                        # word 2: the in side's W_S from K20 side [1]; word 10 the out side's from [0]
    assert int(r[7]) == 40_959 * (1 + 2 ** 32) and int(r[15]) == 2_047 * (1 + 2 ** 32)   # r = 419430 -> 40959.9; r = 20971 -> 2047.9
    assert int(r[16]) == 4 | 16


def test_a_per_key_objective_and_its_reset():
    ref = SloRef("group_nodes", 8, 2, 4, **P)
    strict = engine.slo_objective(1, 999_000, 999_990)               # bin 1, budgets 1000 and 10 ppm
    assert strict == 1 << 28 | 1000 << 12 | 10 and objective_ok(strict)   # the smallest exponent that holds the budget: 1000 x 10^0, 10 x 10^0
    ref.assign([G(2)], [strict])
    rows = [(G(2), 100, 1, 0, 0), (5, 100, 1, 0, 0)]
    bins = dict(in_bins={0: {2: 10, 5: 5}, 1: {2: 10, 5: 5}})
    a = _close(ref, rows, **bins)
    assert int(a[0][16]) >> 32 == strict and int(a[1][16]) >> 32 == 0
    assert (int(a[0][2]), int(a[1][2])) == (15, 5)                    # bins 2 .. 15 against bins 4 .. 15
    assert int(a[0][6]) & 0xFFFFFFFF == 1_023_925 and int(a[1][6]) & 0xFFFFFFFF == 10_239   # r = 10485: 10 ppm against 1000 ppm
    ref.assign([G(2)], [0])
    b = _close(ref, rows, **bins)
    assert int(b[0][16]) >> 32 == 0 and int(b[0][2]) == 20            # history stays: 15 under the old bin + 5 under the default
    assert b[0][:2].tolist() == b[1][:2].tolist() and int(b[0][6]) == int(b[1][6])
    assert ref.entries()[:, 13].tolist() == [0, 0] and ref.entries()[:, 0].tolist() == [2, 4 + 5]
    for bad in (15 << 28 | 1 << 12 | 1, 1 << 24 | 1 << 12 | 1, 1 << 12, 1, 1001 << 12 | 1, (3 << 10 | 1000) << 12 | 1):
        assert not objective_ok(bad), hex(bad)
    with pytest.raises(ValueError):
        engine.slo_objective(3, 998_999, 999_000)                     # a budget of 1001 ppm has four significant digits
    with pytest.raises(ValueError):
        engine.slo_objective(15, 990_000, 999_000)


def test_untracked_rows_and_keys():
    ref = SloRef("nodes", 8, 2, **P)
    out = _close(ref, [(7, 5, 0, 0, 0), (LABEL | 0, 5, 0, 0, 0), (LABEL | 1, 5, 0, 0, 0), (OBIP | 0, 5, 5, 5, 5)])
    assert (out[3][:16] == 0).all() and int(out[3][16]) == 1 and int(out[3][17]) == 0
    assert ref.entries()[:, 0].tolist() == [7, 8, 9] and ref.key(8) is None and ref.key(LABEL | 2) is None and ref.key(G(0)) is None
    wl = SloRef("group_nodes", 8, 2, 4, **P)
    assert [wl.key(r) for r in (G(0), G(3), G(4), 0, 7, LABEL | 1, OBIP | 0)] == [0, 3, None, 4, 11, 13, None]


def test_the_selection_ranks_by_the_smaller_span_with_ties_by_position():
    rows = np.zeros((5, 18), dtype=np.uint64)
    for k, (short, long_, total, flags) in enumerate(((900, 2000, 50, 0), (3000, 900, 50, 0), (5000, 5000, 5, 0), (0, 0, 0, 1), (1200, 1100, 50, 0))):
        rows[k, 8 + 7] = short | long_ << 32; rows[k, 8 + 3] = total; rows[k, 16] = flags
    assert slo_values(rows, "slow", "out", 10) == [900, 900, 0, 0, 1100]
    assert ref_select_slo(rows, "slow", "out", 2, 0, 10).tolist() == [4, 0] and ref_select_slo(rows, "slow", "out", 0, 900, 10).tolist() == [0, 1, 4]
    assert ref_select_slo(rows, "slow", "out", 5, 901, 10).tolist() == [4] and ref_select_slo(rows, "err", "out", 1, 1, 10).tolist() == []
    assert ref_select_slo(rows, "slow", "out", 3, 0, 0).tolist() == [2, 4, 0]


# ---- 3. the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slo_plan") / "slo_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "micro", "slo_plan_test.cpp")])

    def run(mode, lines):
        text = "".join(" ".join(map(str, l)) + "\n" for l in lines)
        out = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return [json.loads(l) for l in out.stdout.splitlines()]
    return run


def _line(spaces=5, on=5, mk=300, ml=16, mg=300, ncap=380, nc=600, slots=1, ss=40, lbin=3, lt=990_000, et=999_000, S=2, L=12, mb=1024, res=0, mr=10):
    return (spaces, on, mk, ml, mg, ncap, nc, slots, ss, lbin, lt, et, S, L, mb, res, mr)


def test_the_plan_is_the_golden_record(driver):
    gold = json.load(open(os.path.join(HERE, "golden", "slo_plan.json")))
    got = driver("plan", [c["line"] for c in gold["cases"]])
    for c, r in zip(gold["cases"], got):
        assert r == c["plan"], c["name"]
    c3 = {c["name"]: c["plan"] for c in gold["cases"]}["c3_both_l64"]
    assert [s["keys"] for s in c3["sp"]] == [15_064, 20_628] and [s["ring_bytes"] for s in c3["sp"]] == [46_276_608, 63_369_216]


def test_the_plans_sizes_in_64_bits_and_what_is_refused(driver):
    for r, (mk, ml, mg, ncap, nc, slots, L) in zip(driver("plan", [_line(mk=a, ml=b, mg=c, ncap=d, nc=e, slots=s, L=l) for a, b, c, d, e, s, l in (
            (1, 0, 0, 1, 1, 1, 2), (300, 16, 300, 380, 600, 3, 12), (1 << 20, 1 << 19, 1 << 19, 1 << 21, 1 << 21, 2, 64))]),
            ((1, 0, 0, 1, 1, 1, 2), (300, 16, 300, 380, 600, 3, 12), (1 << 20, 1 << 19, 1 << 19, 1 << 21, 1 << 21, 2, 64))):
        assert r["rc"] == 0 and (r["params_size"], r["stats_size"], r["row_words"], r["entry_words"], r["max_windows"]) == (40, 32, 18, 14, 64)
        assert (r["lat_budget"], r["err_budget"]) == (10_000, 1_000)
        for s, keys, cap in zip(r["sp"], (mk + ml, mg + mk + ml), (ncap, nc)):
            assert (s["keys"], s["cap"]) == (keys, cap)
            assert (s["ring_bytes"], s["sums_bytes"], s["obj_bytes"]) == (L * keys * 48, keys * 96, keys * 4)
            assert s["rows_bytes"] >= cap * 144 and s["slot"][1] >= s["rows_bytes"]
            assert s["key_wgs"] == min(1024, -(-keys // 256)) and s["row_wgs"] == min(1024, -(-cap // 256))
            end = 0
            for name, off, size in s["layout"]:                       # the pieces in order, none overlapping, each 256-byte aligned
                assert off >= end and off % 256 == 0, name
                end = off + size
            assert s["total_bytes"] >= end and [p[0] for p in s["layout"]].count("rows") == slots
        assert r["total_bytes"] == sum(s["total_bytes"] for s in r["sp"])
    big = driver("plan", [_line(mk=1 << 20, ml=1 << 19, mg=1 << 19, ncap=1 << 21, nc=1 << 21, L=64)])[0]
    assert big["sp"][1]["ring_bytes"] == 64 * (1 << 21) * 48 > 1 << 32
    one, = driver("plan", [_line(spaces=4, on=5)])
    assert one["spaces"] == 4 and one["sp"][0] is None and one["total_bytes"] == one["sp"][1]["total_bytes"]
    bad = driver("plan", [_line(spaces=0), _line(spaces=2), _line(spaces=7), _line(spaces=8), _line(ss=36), _line(res=1), _line(lbin=15), _line(lt=0),
                          _line(lt=1_000_000), _line(et=0), _line(et=1_000_000), _line(S=0), _line(S=13), _line(S=65, L=65), _line(L=65),
                          _line(spaces=1, mk=(1 << 21) - 15), _line(spaces=4, mk=1 << 20, ml=0, mg=(1 << 20) + 1)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * len(bad)
    ok = driver("plan", [_line(spaces=1, mk=(1 << 21) - 16), _line(spaces=1, mk=1 << 20, ml=0, mg=1 << 30), _line(S=64, L=64), _line(S=1, L=1)])
    assert [r["rc"] for r in ok] == [0] * 4                           # exactly 2^21 keys; the groups do not count for the node space
    off = driver("plan", [_line(spaces=1, on=4), _line(spaces=5, on=1), _line(spaces=4, on=0)])
    assert [r["rc"] for r in off] == [engine.SG_ESTATE] * 3
    assert driver("plan", [_line(spaces=6, on=1)])[0]["rc"] == engine.SG_EINVAL     # unknown bits before the state


def test_the_hosts_objective_check_is_the_references(driver):
    rng = np.random.default_rng(7)
    words = [0, 1, 1 << 12, engine.slo_objective(14, 1000, 999_999), engine.slo_objective(0, 999_999, 1000), 15 << 28 | 1 << 12 | 1, 1 << 24 | 1 << 12 | 1,
             1001 << 12 | 1, (3 << 10 | 1000) << 12 | 1, (3 << 10 | 999) << 12 | (3 << 10 | 999), 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 1 << 32, 400)]
    words += [int(b) << 28 | int(l) << 12 | int(e) for b, l, e in zip(rng.integers(0, 16, 400), rng.integers(0, 4096, 400), rng.integers(0, 4096, 400))]
    got = driver("objective", [(w,) for w in words])
    assert sum(r["ok"] for r in got) > 100
    for w, r in zip(words, got):
        assert r["word"] == w and bool(r["ok"]) == objective_ok(w), hex(w)
    assert (got[3]["bin"], got[3]["lat_budget"], got[3]["err_budget"]) == (14, 999_000, 1)
    assert (got[4]["bin"], got[4]["lat_budget"], got[4]["err_budget"]) == (0, 1, 999_000)


# ---- 4. the header's constants -----------------------------------------------------------------------------------------------------------
def test_the_headers_constants_and_structs_are_the_front_ends(tmp_path):
    with open(os.path.join(ROOT, "include", "servicegraph.h")) as f:
        h = f.read()
    d = {n: int(v) for n, v in re.findall(r"#define\s+(SG_SLO(?:SEL)?_[A-Z_]+)\s+(\d+)u", h)}
    assert d == dict(SG_SLO_WORDS=engine.SLO_WORDS, SG_SLO_MAX_WINDOWS=engine.SLO_MAX_WINDOWS, SG_SLO_ENTRY_WORDS=engine.SLO_ENTRY_WORDS,
                     SG_SLO_UNTRACKED=engine.SLO_UNTRACKED, SG_SLO_ERR_BURNING_IN=engine.SLO_ERR_BURNING_IN,
                     SG_SLO_SLOW_BURNING_IN=engine.SLO_SLOW_BURNING_IN, SG_SLO_ERR_BURNING_OUT=engine.SLO_ERR_BURNING_OUT,
                     SG_SLO_SLOW_BURNING_OUT=engine.SLO_SLOW_BURNING_OUT, SG_SLOSEL_ERR=engine.SLOSEL_BY["err"], SG_SLOSEL_SLOW=engine.SLOSEL_BY["slow"],
                     SG_SLOSEL_IN=engine.SLOSEL_SIDE["in"], SG_SLOSEL_OUT=engine.SLOSEL_SIDE["out"])
    assert set(engine.SLO_DEFAULTS) | {"struct_size", "reserved"} == {f for f, _ in engine.SloParams._fields_}
    assert engine.ABI_VERSION == 6 and "#define SG_ABI_VERSION 6u" in h        # additive: the version does not move
    src = tmp_path / "slo_layout_check.c"
    lines = ['#include <stddef.h>', '#include "servicegraph.h"']
    for struct, ctype in (("sg_slo_params", engine.SloParams), ("sg_slo_stats", engine.SloStats)):
        lines.append(f"_Static_assert(sizeof({struct}) == {C.sizeof(ctype)}, \"{struct}\");")
        for name, t in ctype._fields_:
            off = getattr(ctype, name).offset
            lines.append(f"_Static_assert(offsetof({struct}, {name}) == {off} && sizeof((({struct}*)0)->{name}) == {C.sizeof(t)}, \"{struct}.{name}\");")
    strict = engine.slo_objective(1, 999_000, 999_990)
    lines.append(f"_Static_assert(SG_SLO_OBJECTIVE(1, 1000, 0, 10, 0) == {strict}u, \"SG_SLO_OBJECTIVE\");")
    lines.append(f"_Static_assert(SG_SLO_BUDGET_CODE(500, 2) == {engine.slo_budget_code(50_000)}u, \"SG_SLO_BUDGET_CODE\");")
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert engine.slo_budget_code(1) == 1 and engine.slo_budget_code(999_000) == 3 << 10 | 999 and engine.slo_budget_code(1000) == 1000
