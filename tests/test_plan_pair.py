"""Pass A's tile pairs in the plan (alaz_amd/csrc/sg_plan.hpp: PassA::k1a_pair / k1a_pair_lds, PassAKernel::pair), on the CPU:
tests/micro/plan_driver.cpp, stage pair, prints pass A's choice for a config line and the join tables' sizes.

The paired form of k1a_team_partition (sg_k1_team.h, PAIR = 1) keeps a second tile's worth of records per team in LDS.  The plan takes it only BESIDE the geometry it chose without pairs — the same cache,
the same level-2 placement —, so every size recorded in tests/golden/plans.json stays what it was; a launch asks for k1a_lds +
k1a_pair_lds bytes.  kernel_lds() below restates the kernel's own carve of that LDS (the pointer arithmetic at the top of
k1a_team_partition), not the plan's sum."""
import pytest

from tests import plan_driver
from tests.plan_driver import run_named as run, stage_fixture

LDS_CAP = 160 * 1024
K1A_TEAM = 3

C2 = "max_known_nodes=1500 max_edges=66596 layers=1 max_labels=64 max_window_events=1000000 k1_variant=3"      # (by name: auto keeps C2 on 16-byte records)
C3 = "max_known_nodes=15000 max_edges=1254096 layers=2 max_labels=64 max_window_events=10000000"                  # the flagship shape
C5_SHARD = "max_known_nodes=150000 max_edges=785346 layers=2 max_labels=64 max_window_events=625000 flags=2"     # 18-bit endpoints
GPU_TEST = "max_known_nodes=2208 max_edges=32768 layers=1 max_labels=64 max_outbound_ips=512 max_window_events=262144 k1_variant=3 SG_NWG=8"
# the join tables of the benchmark's C3 engine (10 000 pod and 5 000 service addresses: 60 /24s): level 1 of 512 entries, 61 level-2 blocks of 1 KiB
C3_FULL = f"{C3} l1=512 l2=62464"
# ... and the same engine with its records arriving split: 1 024 partitions of one pass-B table each instead of 512 of two sub-tables
C3_SPLIT = f"{C3_FULL} SG_NP=1024 SG_SPLIT=1 SG_HT=2048"


pair_exe = stage_fixture("pair")


def kernel_lds(r, pair):
    """bytes k1a_team_partition<..., PAIR> addresses, from its own pointer arithmetic: fcn | fcw | tcnt[teams][4][np] | red[8] | bar[16] |
    tiles[teams][tile + 2] (+ the pad that keeps 16-byte alignment: the kernel adds 4 words whatever the teams; PAIR: twice the tile)
    | the join blob (level 1 as it is; level 2, if staged, as u32 or packed to u16), rounded to 16 | ckey[ct] | cacc[ct][4]"""
    np_, teams, nt, ct = r["np"], r["k1a_teams"], r["k1a_nt"], r["k1a_ct"]
    tile = (2 if pair else 1) * (4 * nt // teams)
    off = np_ * 4 * 2 + teams * 4 * np_ * 4 + 8 * 8 + 16 * 4
    off += (teams * tile + 4) * 8
    assert off % 16 == 0
    l1b = r["l1_entries"] * 8
    jl = l1b + ((r["l2_bytes"] // 2 if r["l2_u16"] else r["l2_bytes"]) if r["l2_in_lds"] else 0)
    off += (jl + 15) // 16 * 16
    return off + ct * 8 + ct * 32


SHAPES = [("c2", C2), ("c3", C3), ("c3_full", C3_FULL), ("c5_shard", C5_SHARD), ("np256", GPU_TEST), ("np512", f"{GPU_TEST} SG_NP=512")]


@pytest.mark.parametrize("knob", ["", " SG_K1A_PAIR=1", " SG_K1A_PAIR=0"])
def test_the_plans_lds_sum_is_the_kernels_layout(pair_exe, knob):
    got = run(pair_exe, [f"{n} {line}{knob}" for n, line in SHAPES])
    for name, _ in SHAPES:
        r = got[name]
        assert r["rc"] == 0 and r["narrow"] == 1 and r["k1a_team"] == 1, (name, r)
        assert r["k1a_lds"] == kernel_lds(r, pair=False), (name, r)
        assert r["k1a_lds"] + r["k1a_pair_lds"] == kernel_lds(r, pair=bool(r["k1a_pair"])), (name, r)
        assert r["k1a_lds"] + r["k1a_pair_lds"] <= LDS_CAP == r["lds_cap"], (name, r)
        assert (r["k1a_pair_lds"] != 0) == bool(r["k1a_pair"]) == bool(r["kernel"]["pair"]), (name, r)
        if knob.endswith("=0"):
            assert r["k1a_pair"] == 0, (name, r)
    # the shapes the paired form exists for take it when asked by name; 18-bit endpoints leave a parked record no room for its partition number
    if knob.endswith("=1"):
        assert [n for n, _ in SHAPES if got[n]["k1a_pair"]] == ["c2", "c3", "c3_full", "np256", "np512"]
        assert got["c3_full"]["k1a_lds"] == 129696 and got["c3_full"]["k1a_pair_lds"] == 32768      # the budget the form was sized on: 1 376 bytes to spare
        assert got["np256"]["np"] == 256 and got["np512"]["np"] == 512
    if knob == "":
        want = got["c3"]["pair_default"]
        assert [got[n]["k1a_pair"] for n in ("c2", "c3", "c3_full", "np256", "np512")] == [want] * 5
    assert got["c5_shard"]["k1a_pair"] == 0 and got["c5_shard"]["nb"] == 18


def test_pairs_change_nothing_else_of_pass_a(pair_exe):
    lines = [f"{n}_{k} {line} SG_K1A_PAIR={k}" for n, line in SHAPES for k in (0, 1)]
    got = run(pair_exe, lines)
    for n, _ in SHAPES:
        a, b = got[f"{n}_0"], got[f"{n}_1"]
        same = ("np", "nb", "l2_u16", "l2_in_lds", "k1a_team", "k1a_ct", "k1a_lds")
        assert [a[k] for k in same] == [b[k] for k in same], n
        assert {k: v for k, v in a["kernel"].items() if k != "pair"} == {k: v for k, v in b["kernel"].items() if k != "pair"}


def test_large_join_tables_fall_back_to_single_tiles(pair_exe):
    """Level 2 grows with the IP blocks in use.  As it does the plan first shrinks the cache; pairs are kept only while they fit beside
    the cache it chose, and by default only beside 512 slots or more — never by shrinking the cache or moving level 2 out of LDS.
    (Level 2 as u16 entries is at most 47 KiB: only an engine of more than 16 384 nodes, whose level 2 is staged as u32, can have its
    cache pushed under 512 slots — the second shape.)"""
    big = C3.replace("max_known_nodes=15000", "max_known_nodes=20000")
    sizes = [(C3, 1024 * k) for k in (1, 30, 60, 70, 80, 90, 100, 110, 120, 140)] + [(big, 1024 * k) for k in (40, 60, 70, 80, 88, 94)]
    names = [f"{i}" for i in range(len(sizes))]
    got = run(pair_exe, [f"d{n} {c} l1=256 l2={l2}" for n, (c, l2) in zip(names, sizes)] + [f"f{n} {c} l1=256 l2={l2} SG_K1A_PAIR=1" for n, (c, l2) in zip(names, sizes)] +
              [f"o{n} {c} l1=256 l2={l2} SG_K1A_PAIR=0" for n, (c, l2) in zip(names, sizes)])
    seen, small_cache = set(), 0
    for l2 in names:
        d, f, o = got[f"d{l2}"], got[f"f{l2}"], got[f"o{l2}"]
        for r in (d, f):
            assert r["k1a_lds"] + r["k1a_pair_lds"] <= LDS_CAP
            assert r["k1a_lds"] + r["k1a_pair_lds"] == kernel_lds(r, pair=bool(r["k1a_pair"]))
        same = ("k1a_ct", "l2_in_lds", "k1a_lds", "k1a_team")
        assert [d[k] for k in same] == [o[k] for k in same], l2          # the default never moves the cache or level 2
        fits = o["k1a_team"] == 1 and o["k1a_lds"] + 32768 <= LDS_CAP
        assert d["k1a_pair"] == int(fits and d["k1a_ct"] >= 512 and d["pair_default"]), (l2, d)
        # by name the one trade is made: a cache of 1 024 slots for 512 where that lets the second tile in
        trade = o["k1a_team"] == 1 and not fits and o["k1a_ct"] == 1024 and o["k1a_lds"] - 512 * 40 + 32768 <= LDS_CAP
        assert f["k1a_pair"] == int(fits or trade), (l2, f)
        assert [f[k] for k in same] == ([512, o["l2_in_lds"], o["k1a_lds"] - 512 * 40, 1] if trade else [o[k] for k in same]), (l2, f)
        seen.add((bool(fits), bool(trade), d["k1a_ct"] >= 512))
        if o["k1a_ct"] < 512:                                            # a cache the tables pushed under 512 slots: no room for pairs, asked for or not
            assert o["l2_in_lds"] == 1 and not fits and not trade and d["k1a_pair"] == f["k1a_pair"] == 0, (l2, o)
            small_cache += 1
    assert (True, False, True) in seen and (False, True, True) in seen and small_cache >= 1
    small = run(pair_exe, [f"s {C3} l1=256 l2=61440 SG_CT=256", f"t {C3} l1=256 l2=61440 SG_CT=256 SG_K1A_PAIR=1"])
    assert small["s"]["k1a_ct"] == 256 and small["s"]["k1a_pair"] == 0 and small["t"]["k1a_pair"] == 1


def test_arriving_split_takes_pairs_by_name_beside_half_the_cache(pair_exe):
    got = run(pair_exe, [f"d {C3_SPLIT}", f"f {C3_SPLIT} SG_K1A_PAIR=1", f"o {C3_SPLIT} SG_K1A_PAIR=0"])
    d, f, o = got["d"], got["f"], got["o"]
    assert d["np"] == f["np"] == 1024 and d["kernel"]["pb"] == 10
    assert (o["k1a_ct"], o["k1a_lds"], o["k1a_pair"]) == (1024, 150176, 0) and (d["k1a_ct"], d["k1a_lds"], d["k1a_pair"]) == (1024, 150176, 0)
    assert (f["k1a_ct"], f["k1a_lds"], f["k1a_pair"], f["k1a_pair_lds"]) == (512, 129696, 1, 32768) and f["kernel"]["pair"] == 1
    for r in (d, f, o):
        assert r["k1a_lds"] + r["k1a_pair_lds"] == kernel_lds(r, pair=bool(r["k1a_pair"])) <= LDS_CAP


def test_every_key_the_plan_can_choose_is_instantiated(pair_exe):
    dom, = plan_driver.run(pair_exe, (), args=("--domains",))
    assert len(dom["k1a_team"]) == 18 and len(dom["k1a_team_pair"]) == 18
    lines = []
    for n, line in SHAPES:
        for world in (1, 2):
            for i, knob in enumerate(("", " SG_K1A_PAIR=1", " SG_K1A_PAIR=0", " SG_L2_U32=1 SG_K1A_PAIR=1", " SG_L2_GLOBAL=1 SG_K1A_PAIR=1", " SG_NP=1024 SG_K1A_PAIR=1")):
                lines.append(f"{n}_w{world}_k{i} {line}{knob}" + (" world=2 rank=1" if world == 2 else ""))
    got = run(pair_exe, lines)
    assert len(got) == len(lines)
    pairs = 0
    for r in got.values():
        if r["rc"] != 0 or r["kernel"]["family"] != K1A_TEAM:
            continue
        k = r["kernel"]
        key = [k["l2"], k["sharded"], k["pb"]]
        assert key in dom["k1a_team_pair" if k["pair"] else "k1a_team"], (r["name"], key)
        pairs += k["pair"]
    assert pairs >= 10


def test_the_knob_is_the_development_builds():
    from alaz_amd import engine
    assert "SG_K1A_PAIR" in engine.DEV_KNOBS
