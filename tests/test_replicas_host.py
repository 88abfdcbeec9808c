"""CPU tests of the replica outliers (K25): the reference of tests/replica_ref.py against the header's worked example and hand-computed
answers over windows folded here from plain edge lists (node rows, workload rows and K20 histograms as K9, K16 and K20 define them:
sums by endpoint), the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/replica_plan_test.cpp against tests/golden/replica_plan.json)
and the header's constants against alaz_amd/engine.py (whose set_replicas is sg_set_replicas' front end)."""
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
from tests.replica_ref import (ERR, JUDGED, LAT, MEMBER, NONE, TAIL, judge, member_sums, members, qbin, ref_select_replicas, replica_ref,
                               replica_values, resolve)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = (1 << 64) - 1
NO = engine.NO_GROUP
P = dict(min_replicas=3, min_requests=20)


def _bin(ns):
    """K20's bin of a duration: bin 0 below 2^17 ns, bin b from 2^(16 + b), bin 15 from 2^31"""
    return min(max(int(ns).bit_length() - 17, 0), 15)


def _fold(edges, gmap, mk):
    """node rows, workload rows and node histograms of a window of edges (from id, to id, requests, errors, duration each): every
    field a sum by endpoint, the workload key of an id its group or itself"""
    def key(i):
        return G(int(gmap[i])) if int(gmap[i]) != NO else i
    acc, wacc = {}, {}
    for f, t, n, e, d in edges:
        for table, kf, kt in ((acc, f, t), (wacc, key(f), key(t))):
            for k, side in ((kf, "out"), (kt, "in")):
                a = table.setdefault(k, {s: [0, 0, 0, [0] * 16] for s in ("in", "out")})[side]
                a[0] += n; a[1] += e; a[2] = (a[2] + n * d) & M64; a[3][_bin(d)] += n
    def rows(table):
        r = np.zeros(len(table), dtype=NODE_DTYPE)
        h = np.zeros((len(table), 2, 16), dtype=np.uint64)
        for k, ref in enumerate(sorted(table)):
            r[k]["ref"] = ref
            for hs, side in ((0, "out"), (1, "in")):
                c, e, s, b = table[ref][side]
                r[k][side + "_count"], r[k][side + "_err"], r[k][side + "_sum_ns"] = c, e, s
                h[k, hs] = b
        return r, h
    (nodes, hist), (wrows, whist) = rows(acc), rows(wacc)
    return nodes, hist, wrows, whist


def _world(n_members=4, extra=6):
    """ids 0 .. n_members - 1: the pods of workload 0; the next `extra`: ungrouped client pods; the last id a Service"""
    mk = n_members + extra + 1
    gmap = np.full(mk, NO, np.uint32); gmap[:n_members] = 0
    kinds = np.full(mk, 1, np.uint8); kinds[mk - 1] = 2
    return mk, gmap, kinds


def _pod(pods, nodes, ref):
    return pods[int(np.flatnonzero(nodes["ref"] == ref)[0])].tolist()


# ---- 1. the worked example -----------------------------------------------------------------------------------------------------------------
def test_the_headers_worked_example_to_the_digit():
    mk, gmap, kinds = _world()
    client = 4
    edges = [(client, 0, 90, 0, 4_000_000), (client, 0, 10, 10, 4_000_000)]
    for pod in (1, 2, 3):
        edges += [(client, pod, 99, 0, 1_000_000), (client + 1, pod, 1, 1, 1_000_000)]
    nodes, hist, wrows, _ = _fold(edges, gmap, mk)
    pods, groups = replica_ref(nodes, wrows, hist, gmap, kinds, P)
    a = _pod(pods, nodes, 0)
    w = int(np.flatnonzero(wrows["ref"] == G(0))[0])
    assert a[0] == w and a[1] == MEMBER | JUDGED | ERR | LAT
    assert a[2:7] == [94372, 4096, 1024, 0, 4]                        # x_err 104857 - 10485; 4 ms over 1 ms; the fair share; no tails; R
    assert (104857, 10485) == ((10 << 20) // 100, (3 << 20) // 300)
    b = _pod(pods, nodes, 1)
    assert b[1] == MEMBER | JUDGED and b[2] == (10485 - ((12 << 20) // 300)) & NONE and b[3] == 1024 * 1_000_000 // 2_000_000
    assert a[7:12] == [0, 0, 0, 0, 0]                                 # the out side: no member sends
    assert groups[w].tolist() == [4, 4, 1, int(np.flatnonzero(nodes["ref"] == 0)[0]), 0, 0, 0, NONE]
    clients = pods[np.isin(nodes["ref"], [4, 5])]
    assert (clients[:, 0] == NONE).all() and (clients[:, 1:] == 0).all()   # ungrouped pods: no members
    assert pods.dtype == np.uint32 and pods.shape == (len(nodes), 12) and groups.shape == (len(wrows), 8)


# ---- 2. the member sums against the workload row -------------------------------------------------------------------------------------------
def test_member_sums_are_the_workload_rows_sums_unless_a_bound_service_is_in_the_group():
    rng = np.random.default_rng(25)
    mk, gmap, kinds = _world(6, 5)
    svc = mk - 1
    edges = [(int(rng.integers(0, mk - 1)), int(rng.integers(0, mk - 1)), int(rng.integers(1, 50)), int(rng.integers(0, 3)), int(1 << rng.integers(10, 34)))
             for _ in range(200)]
    edges = [(f, t, n, min(e, n), d) for f, t, n, e, d in edges if f != t]
    for tails in (0, 990):
        nodes, hist, wrows, whist = _fold(edges, gmap, mk)
        w = int(np.flatnonzero(wrows["ref"] == G(0))[0])
        s = member_sums(nodes, wrows, hist if tails else None, gmap, kinds)[w]
        for hs, side in ((0, "out"), (1, "in")):
            R, Cc, E, T, H = s[side]
            assert (Cc, E, T) == tuple(int(wrows[w][side + x]) for x in ("_count", "_err", "_sum_ns")), side
            assert 0 < R <= 6
            if tails:
                assert H == [int(x) for x in whist[w, hs]]
    bound = gmap.copy(); bound[svc] = 0                               # service binding puts the Service into the group
    edges2 = edges + [(7, svc, 40, 2, 1 << 20)]
    nodes, hist, wrows, whist = _fold(edges2, bound, mk)
    w = int(np.flatnonzero(wrows["ref"] == G(0))[0])
    mem = members(nodes, wrows, bound, kinds)
    assert mem[int(np.flatnonzero(nodes["ref"] == svc)[0])] is None and mem.count(w) == 6
    s = member_sums(nodes, wrows, hist, bound, kinds)[w]
    assert s["in"][1] == int(wrows[w]["in_count"]) - 40 and s["in"][4] != [int(x) for x in whist[w, 1]]
    pods, _ = replica_ref(nodes, wrows, hist, bound, kinds, P)
    assert _pod(pods, nodes, svc) == [NONE] + [0] * 11
    lab = nodes.copy(); lab["ref"][0] |= 1 << 30                      # a LABEL and an OBIP ref with a grouped id's value: never members
    assert members(lab, wrows, bound, kinds)[0] is None
    lab["ref"][0] = nodes["ref"][0] | 2 << 30
    assert members(lab, wrows, bound, kinds)[0] is None


# ---- 3. each threshold at its value and one below ------------------------------------------------------------------------------------------
def _close(calls, params, n_members=4, tails=False):
    """one window: calls = {member pod: (requests, errors, duration)} from one client each"""
    mk, gmap, kinds = _world(n_members)
    edges = [(n_members, pod, n, e, d) for pod, (n, e, d) in calls.items()]
    nodes, hist, wrows, _ = _fold(edges, gmap, mk)
    pods, groups = replica_ref(nodes, wrows, hist, gmap, kinds, params)
    return {pod: _pod(pods, nodes, pod) for pod in calls}, groups[int(np.flatnonzero(wrows["ref"] == G(0))[0])].tolist()


def test_min_requests_on_the_pod_and_on_its_peers_and_min_replicas():
    rows, _ = _close({0: (19, 0, 1000), 1: (20, 0, 1000), 2: (20, 0, 1000)}, P)
    assert rows[0][1] == MEMBER and rows[0][2:7] == [0, 0, 0, 0, 3]   # c = 19: not judged, every value 0, R reported
    assert rows[1][1] == MEMBER | JUDGED and rows[2][1] == MEMBER | JUDGED
    rows, _ = _close({0: (30, 0, 1000), 1: (10, 0, 1000), 2: (9, 0, 1000)}, P)
    assert rows[0][1] == MEMBER                                       # its peers have 19
    rows, _ = _close({0: (30, 0, 1000), 1: (10, 0, 1000), 2: (10, 0, 1000)}, P)
    assert rows[0][1] == MEMBER | JUDGED and rows[1][1] == MEMBER     # its peers have 20; pod 1 itself has 10
    rows, g = _close({0: (30, 0, 1000), 1: (30, 0, 1000)}, P)
    assert rows[0][1] == MEMBER and g[:4] == [2, 0, 0, NONE]          # R = min_replicas - 1
    rows, g = _close({0: (30, 0, 1000), 1: (30, 0, 1000), 2: (1, 0, 1000)}, P)
    assert rows[0][1] == MEMBER | JUDGED and rows[2][1] == MEMBER and g[:4] == [3, 2, 0, NONE]   # the third replica is active, not judged
    rows, _ = _close({0: (30, 0, 1000), 1: (30, 0, 1000)}, dict(min_replicas=2))
    assert rows[0][1] == MEMBER | JUDGED
    assert resolve({}) == dict(min_replicas=3, min_requests=20, min_err_excess_q20=20972, min_lat_ratio_q10=2048, tail_permille=0, min_tail_bins=2)


def test_each_flags_threshold_at_the_value_and_one_below():
    calls = {0: (100, 7, 3_000_000), 1: (100, 1, 1_000_000), 2: (100, 1, 1_000_000), 3: (100, 1, 1_000_000)}
    rows, _ = _close(calls, P)
    excess, ratio = rows[0][2], rows[0][3]
    assert excess == (7 << 20) // 100 - (3 << 20) // 300 == 62915 and ratio == 3072
    for thr, flag in ((excess, ERR), (excess + 1, 0)):
        rows, _ = _close(calls, dict(P, min_err_excess_q20=thr, min_lat_ratio_q10=1 << 20))
        assert rows[0][1] == MEMBER | JUDGED | flag
    for thr, flag in ((ratio, LAT), (ratio + 1, 0)):
        rows, g = _close(calls, dict(P, min_err_excess_q20=1 << 20, min_lat_ratio_q10=thr))
        assert rows[0][1] == MEMBER | JUDGED | flag and g[2] == (1 if flag else 0)
    assert rows[1][2] == ((1 << 20) // 100 - (9 << 20) // 300) & NONE and rows[1][2] >= 1 << 31   # a replica below its peers: negative, never ERR
    # tails: pod 0's requests sit three bins above its peers' (the LAT threshold is out of reach, so that TAIL stands alone)
    tail = {0: (100, 0, 1 << 23), 1: (100, 0, 1 << 20), 2: (100, 0, 1 << 20), 3: (100, 0, 1 << 20)}
    for bins, flag in ((3, TAIL), (4, 0)):
        rows, _ = _close(tail, dict(P, tail_permille=990, min_tail_bins=bins, min_lat_ratio_q10=1 << 20), tails=True)
        assert rows[0][5] == _bin(1 << 23) | _bin(1 << 20) << 8 and rows[0][1] == MEMBER | JUDGED | flag
    rows, _ = _close(tail, dict(P, min_lat_ratio_q10=1 << 20))        # tails off: the word is 0 whatever the histograms hold
    assert rows[0][5] == 0 and rows[0][1] == MEMBER | JUDGED
    assert qbin([0] * 16, 990) == 0 and qbin([99, 1] + [0] * 14, 990) == 0 and qbin([98, 2] + [0] * 14, 990) == 1 and qbin([1] + [0] * 15, 1) == 0


def test_a_tail_only_outlier_with_the_mean_ratio_below_its_threshold():
    mk, gmap, kinds = _world()
    edges = [(4, 0, 97, 0, 1 << 20), (4, 0, 3, 0, 1 << 22)]           # 3 % of pod 0's requests two octaves up: p99 moves, the mean barely
    edges += [(4, pod, 100, 0, 1 << 20) for pod in (1, 2, 3)]
    nodes, hist, wrows, _ = _fold(edges, gmap, mk)
    pods, groups = replica_ref(nodes, wrows, hist, gmap, kinds, dict(P, tail_permille=990))
    a = _pod(pods, nodes, 0)
    assert a[1] == MEMBER | JUDGED | TAIL and a[3] < 2048 and a[5] == 6 | 4 << 8
    assert replica_values(pods, "tail", "in")[int(np.flatnonzero(nodes["ref"] == 0)[0])] == 2


# ---- 4. the clamp and the wrap ----------------------------------------------------------------------------------------------------------------
def test_a_request_of_two_to_the_sixty_and_two_of_two_to_the_sixty_three():
    big = {0: (15, 0, 1 << 60), 1: (20, 0, 1 << 40), 2: (20, 0, 1 << 40), 3: (20, 0, 1 << 40)}   # 15 x 2^60 < 2^64: the sum does not wrap
    P = dict(min_replicas=3, min_requests=15)
    rows, _ = _close(big, P)
    assert rows[0][3] == (1 << 52) * 1024 >> 40 == 1 << 22            # the mean is clamped at 2^52: 2^30 without the clamp
    rows, _ = _close({**big, 1: (20, 0, 1), 2: (20, 0, 1), 3: (20, 0, 1)}, P)
    assert rows[0][3] == NONE                                         # 2^62 is clamped to a u32
    # pods 1 and 3 each served one request of 2^63 ns: T wraps past them, and T - S wraps back
    mk, gmap, kinds = _world()
    edges = [(4, pod, 19, 0, 1000) for pod in (1, 3)] + [(5, pod, 1, 0, 1 << 63) for pod in (1, 3)] + [(4, 0, 20, 0, 1000), (4, 2, 20, 0, 900)]
    nodes, hist, wrows, _ = _fold(edges, gmap, mk)
    w = int(np.flatnonzero(wrows["ref"] == G(0))[0])
    T = member_sums(nodes, wrows, None, gmap, kinds)[w]["in"][3]
    assert T == 2 * 19_000 + 20_000 + 18_000 and int(wrows[w]["in_sum_ns"]) == T      # both 2^63 are gone from the sum
    pods, _ = replica_ref(nodes, wrows, hist, gmap, kinds, P)
    one = _pod(pods, nodes, 1)
    assert int(nodes[int(np.flatnonzero(nodes["ref"] == 1)[0])]["in_sum_ns"]) == (1 << 63) + 19_000 > T
    peers = (T - ((1 << 63) + 19_000)) & M64                          # = 2^63 + 57 000: pods 0, 2 and 3 for real
    assert peers == (1 << 63) + 57_000
    assert one[3] == min(((1 << 63) + 19_000) // 20, 1 << 52) * 1024 // min(peers // 60, 1 << 52) == 1024
    zero = _pod(pods, nodes, 0)
    assert zero[3] == 1000 * 1024 // min(((T - 20_000) & M64) // 60, 1 << 52)       # its peers' sum wrapped to 56 000: mean 933
    assert zero[3] == 1000 * 1024 // 933
    f, excess, ratio, share, tp, tq = judge(1 << 60, 1 << 59, 5, [0] * 16, 3, 1 << 61, 1 << 59, 9, [0] * 16, resolve(P))
    assert excess == 1 << 19 and share == min((1 << 53) * 1024 // ((1 << 61) // 3), NONE)   # c is capped at 2^53 in the share


# ---- 5. the selection's reference --------------------------------------------------------------------------------------------------------------
def test_the_selection_keys_and_ties_by_position():
    pods = np.zeros((6, 12), np.uint32)
    pods[:, 0] = [0, 0, 0, NONE, 1, 1]
    pods[:, 1] = [MEMBER | JUDGED, MEMBER | JUDGED | ERR, MEMBER, 0, MEMBER | JUDGED << 4, MEMBER | JUDGED]
    pods[:, 2] = [5, 70, 900, 0, 0, (-3) & NONE]
    pods[:, 4] = [1024, 1024, 4000, 0, 0, 0]
    pods[4, 7:10] = [9, 8, 7]
    assert replica_values(pods, "err", "in") == [5, 70, 0, 0, 0, 0]   # not judged: 0; negative: 0
    assert replica_values(pods, "share", "in") == [1024, 1024, 0, 0, 0, 0] and replica_values(pods, "err", "out") == [0, 0, 0, 0, 9, 0]
    assert ref_select_replicas(pods, "err", "in", 1, 0).tolist() == [1] and ref_select_replicas(pods, "err", "in", 0, 0).tolist() == [0, 1]
    assert ref_select_replicas(pods, "share", "in", 1, 0).tolist() == [0] and ref_select_replicas(pods, "err", "in", 5, 6).tolist() == [1]
    assert ref_select_replicas(pods, "lat", "out", 0, 0).tolist() == [4]


# ---- 6. the plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replica_plan") / "replica_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "micro", "replica_plan_test.cpp")])

    def run(lines):
        text = "".join(" ".join(map(str, l)) + "\n" for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return [json.loads(l) for l in out.stdout.splitlines()]
    return run


def _line(world=1, up=15, ncap=380, gk=680, nc=600, slots=1, ss=40, mrep=0, mreq=0, merr=0, mlat=0, tail=0, mtail=0, r0=0, r1=0):
    return (world, up, ncap, gk, nc, slots, ss, mrep, mreq, merr, mlat, tail, mtail, r0, r1)


def test_the_plan_is_the_golden_record(driver):
    gold = json.load(open(os.path.join(HERE, "golden", "replica_plan.json")))
    got = driver([c["line"] for c in gold["cases"]])
    for c, r in zip(gold["cases"], got):
        assert r == c["plan"], c["name"]
    c3 = {c["name"]: c["plan"] for c in gold["cases"]}
    assert (c3["c3_tails"]["range_rows"], c3["c3_tails"]["ranges"], c3["c3_tails"]["slices"]) == (204, 104, 8)
    assert (c3["c3_no_tails"]["range_rows"], c3["c3_no_tails"]["ranges"], c3["c3_no_tails"]["slices"]) == (1024, 21, 8)


def test_the_plans_sizes_defaults_and_what_is_refused(driver):
    cases = [(380, 680, 600, 1, 0), (380, 680, 600, 3, 990), (1, 1, 1, 1, 0), (1 << 21, 1 << 21, 1 << 21, 2, 999)]
    for r, (ncap, gk, nc, slots, tail) in zip(driver([_line(ncap=a, gk=b, nc=c, slots=s, tail=t) for a, b, c, s, t in cases]), cases):
        assert r["rc"] == 0 and (r["params_size"], r["row_words"], r["group_row_words"]) == (40, 12, 8)
        assert r["params"] == dict(min_replicas=3, min_requests=20, min_err_excess_q20=20972, min_lat_ratio_q10=2048, tail_permille=tail, min_tail_bins=2)
        words = 40 if tail else 8
        assert (r["tails"], r["words"], r["range_rows"]) == (int(tail != 0), words, 65536 // (8 * words))
        assert r["lds_bytes"] == r["range_rows"] * words * 8 <= 65536 and r["vlds_bytes"] == r["range_rows"] * 48   # two workgroups a CU of 160 KiB
        assert r["ranges"] == -(-nc // r["range_rows"]) and 1 <= r["slices"] <= 64
        assert r["slices"] == max(1, min(64, -(-ncap // 2048), (256 << 20) // (r["ranges"] * r["lds_bytes"])))
        assert r["part_bytes"] == r["ranges"] * r["slices"] * r["lds_bytes"] <= max(256 << 20, r["ranges"] * r["lds_bytes"])
        assert r["vpart_bytes"] == r["ranges"] * r["slices"] * r["vlds_bytes"] and r["wsum_bytes"] == nc * words * 8
        assert r["pod_bytes"] >= ncap * 48 and r["group_bytes"] >= nc * 32 and r["slot"][1] >= r["pod_bytes"] + r["group_bytes"]
        assert r["node_wgs"] == min(1024, -(-ncap // 256)) and r["group_wgs"] == min(1024, -(-nc // 256))
        end = 0
        for name, off, size in r["layout"]:                           # the pieces in order, none overlapping, each 256-byte aligned
            assert off >= end and off % 256 == 0, name
            end = off + size
        names = [p[0] for p in r["layout"]]
        assert r["total_bytes"] >= end and names.count("pod_rows") == names.count("group_rows") == slots
        sizes = {p[0]: p[2] for p in r["layout"]}
        assert sizes["pos"] >= gk * 4 and sizes["tgt"] >= ncap * 4 and sizes["stage"] == 1024 * 48
    given, = driver([_line(mrep=2, mreq=1, merr=1 << 20, mlat=1, tail=1, mtail=15)])
    assert given["params"] == dict(min_replicas=2, min_requests=1, min_err_excess_q20=1 << 20, min_lat_ratio_q10=1, tail_permille=1, min_tail_bins=15)
    bad = driver([_line(ss=36), _line(r0=1), _line(r1=1), _line(mrep=1), _line(merr=(1 << 20) + 1), _line(tail=1000), _line(mtail=16), _line(world=2),
                  _line(gk=(1 << 21) + 1), _line(world=2, up=0)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * len(bad)
    off = driver([_line(up=6), _line(up=5), _line(up=3), _line(up=7, tail=990), _line(up=0)])
    assert [r["rc"] for r in off] == [engine.SG_ESTATE] * len(off)    # the nodes, the groups, the workload rows; K20's node space for tails
    assert driver([_line(up=7)])[0]["rc"] == 0                        # without tails K20 is not asked for


# ---- 7. the header's constants -------------------------------------------------------------------------------------------------------------
def test_the_headers_constants_and_struct_are_the_front_ends(tmp_path):
    with open(os.path.join(ROOT, "include", "servicegraph.h")) as f:
        h = f.read()
    d = {n: int(v) for n, v in re.findall(r"#define\s+(SG_(?:REPLICA|REPL|RSEL)_[A-Z_]+)\s+(\d+)u", h)}
    assert d == dict(SG_REPLICA_WORDS=engine.REPLICA_WORDS, SG_REPLICA_GROUP_WORDS=engine.REPLICA_GROUP_WORDS, SG_REPL_MEMBER=engine.REPL_MEMBER,
                     SG_REPL_JUDGED_IN=engine.REPL_JUDGED_IN, SG_REPL_ERR_IN=engine.REPL_ERR_IN, SG_REPL_LAT_IN=engine.REPL_LAT_IN,
                     SG_REPL_TAIL_IN=engine.REPL_TAIL_IN, SG_REPL_JUDGED_OUT=engine.REPL_JUDGED_OUT, SG_REPL_ERR_OUT=engine.REPL_ERR_OUT,
                     SG_REPL_LAT_OUT=engine.REPL_LAT_OUT, SG_REPL_TAIL_OUT=engine.REPL_TAIL_OUT, SG_RSEL_ERR=engine.RSEL_BY["err"],
                     SG_RSEL_LAT=engine.RSEL_BY["lat"], SG_RSEL_TAIL=engine.RSEL_BY["tail"], SG_RSEL_SHARE=engine.RSEL_BY["share"],
                     SG_RSEL_IN=engine.RSEL_SIDE["in"], SG_RSEL_OUT=engine.RSEL_SIDE["out"])
    assert (MEMBER, JUDGED, ERR, LAT, TAIL) == (engine.REPL_MEMBER, engine.REPL_JUDGED_IN, engine.REPL_ERR_IN, engine.REPL_LAT_IN, engine.REPL_TAIL_IN)
    assert engine.REPL_JUDGED_OUT == JUDGED << 4 and engine.REPL_TAIL_OUT == TAIL << 4
    assert set(engine.REPLICA_DEFAULTS) | {"struct_size", "reserved"} == {f for f, _ in engine.ReplicaParams._fields_}
    assert engine._STAGES["replicas"].call == "sg_set_replicas" and "sg_set_replicas" in engine._signatures()
    assert engine.ABI_VERSION == 6 and "#define SG_ABI_VERSION 6u" in h        # additive: the version does not move
    src = tmp_path / "replica_layout_check.c"
    lines = ['#include <stddef.h>', '#include "servicegraph.h"']
    struct, ctype = "sg_replica_params", engine.ReplicaParams
    lines.append(f"_Static_assert(sizeof({struct}) == {C.sizeof(ctype)}, \"{struct}\");")
    for name, t in ctype._fields_:
        off = getattr(ctype, name).offset
        lines.append(f"_Static_assert(offsetof({struct}, {name}) == {off} && sizeof((({struct}*)0)->{name}) == {C.sizeof(t)}, \"{struct}.{name}\");")
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
