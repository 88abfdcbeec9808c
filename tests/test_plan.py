"""The engine's launch plan (alaz_amd/csrc/sg_plan.hpp) on the CPU: tests/micro/plan_driver.cpp, stage plan, prints the plan of every case of
tests/golden/plans.json, which holds the sizing decisions the engine made at commit 38499a0 — before the planner existed —
recorded on an MI355X from that commit's own sg_create, with and without the development build's SG_* overrides."""
import json
import os

from tests import plan_driver
from tests.plan_driver import run_named as run_plans, stage_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plans.json")


plan_exe = stage_fixture("plan")


def planner_input(case):
    """the case's config and overrides; the recorded join-table sizes after the upserts instead of the upserts themselves"""
    toks = [t for t in case["input"].split() if t.split("=")[0] not in ("pods", "svcs", "per")]
    after = case["result"].get("pass_a_after")
    if after:
        toks += [f"l1={after['l1_entries']}", f"l2={after['l2_bytes']}"]
    return " ".join([case["name"], f"cus={case['result'].get('cus', 256)}"] + toks)


def test_plans_match_the_engine_they_replace(plan_exe):
    doc = json.load(open(GOLDEN))
    cases = doc["cases"]
    assert len(cases) >= 100
    got = run_plans(plan_exe, [planner_input(c) for c in cases])
    bad = []
    for c in cases:
        want, have = c["result"], got[c["name"]]
        if c["name"] == "knob_SG_DH_G_warm":
            # the one intended change: SG_DH_G no longer switches the degree histogram on for an engine that keeps warm state
            assert want["plan"]["warm"] == 1 and want["plan"]["dh_g"] == 32
            want = json.loads(json.dumps(want))
            want["plan"].update(dh_g=0, dh_ppw=0, dh_ns=0)
        assert have["rc"] == want["rc"], c["name"]
        for part in ("plan", "pass_a", "pass_a_after"):
            if part not in want:
                continue
            assert set(have[part]) == set(want[part]), (c["name"], part, set(have[part]) ^ set(want[part]))
            bad += [(c["name"], part, k, want[part][k], have[part][k]) for k in want[part] if want[part][k] != have[part][k]]
        if "upsert_rc" in want:
            assert have["upsert_rc"] == want["upsert_rc"], c["name"]
    assert not bad, bad[:20]


def test_dh_g_override_leaves_a_warm_engine_on_degree_atomics(plan_exe):
    base = "max_known_nodes=15000 max_edges=1254096 layers=2 max_labels=64 max_window_events=10000000"
    r = run_plans(plan_exe, [f"warm {base} SG_DH_G=32", f"cold {base} flags=2 SG_DH_G=32"])
    assert r["warm"]["plan"]["warm"] == 1 and r["warm"]["plan"]["dh_g"] == 0
    assert r["cold"]["plan"]["warm"] == 0 and r["cold"]["plan"]["dh_g"] == 32


def test_k6_one_wg_knob_reaches_the_plan_of_a_sharded_engine(plan_exe):
    """tests/test_gpu_halo.py compares the one-workgroup halo-list builders with k6_halo_lists: that is a comparison of two kernels only
    while SG_K6_ONE_WG=1 sets plan.k6_one_wg (the one field launch_halo_lists branches on) and nothing else does — at the node
    capacities either side of the builder's LDS staging that the GPU test uses."""
    cases = {"small": "max_known_nodes=180 max_labels=3072 max_outbound_ips=512", "big": "max_known_nodes=180 max_labels=50176 max_outbound_ips=512"}
    lines = [f"{n}_{k} {c} max_edges=16384 layers=2 rank=1 world=8 max_window_events=65536" + (" SG_K6_ONE_WG=1" if k == "on" else "")
             for n, c in cases.items() for k in ("on", "off")]
    r = run_plans(plan_exe, lines)
    for n in cases:
        assert r[f"{n}_on"]["rc"] == r[f"{n}_off"]["rc"] == 0
        assert r[f"{n}_on"]["plan"]["k6_one_wg"] == 1 and r[f"{n}_off"]["plan"]["k6_one_wg"] == 0
        assert {k for k, v in r[f"{n}_on"]["plan"].items() if r[f"{n}_off"]["plan"][k] != v} == {"k6_one_wg"}
    assert r["small_on"]["plan"]["ncap"] <= 49152 < r["big_on"]["plan"]["ncap"]


def test_knob_list_is_the_engines(plan_exe):
    from alaz_amd import engine
    out = plan_driver.run_text(plan_exe, args=("--knobs",))
    assert tuple(out.split()) == engine.DEV_KNOBS


K1A_GLOBAL, K1A_WIDE, K1A_TILE, K1A_TEAM = range(4)
K1B_NONE, K1B_MERGE, K1B_STREAM = range(3)
LDS_BYTES = 160 * 1024


def ladder_choice(plan, pa, world, cus):
    """The kernel instantiation each launch site took before the choice was a plan field: the launch ladders of servicegraph.hip at
    commit 69acf5a, restated over the plan and pass-A fields the driver prints.  A field the chosen kernel does not take is 0.

    - pass A, launch_k1, lines 307-338: `sh` = world > 1; narrow and k1a_team: K1M_GO (312-314: np 256 -> 8, 512 -> 9, anything else
      -> 10) under the level-2 chain of 328-330 (l2_in_lds and l2_u16 -> 2, l2_in_lds -> 1, else 0); narrow: K1T_GO2 (311: nsub == 2 -> 2,
      else 1) under the same chain, 333-335; else K1A_GO2 (309: hist) with l2_in_lds as a boolean, 337-338; variant 1 launches
      k1_resolve_aggregate, 349.
    - pass B, do_close, lines 442-464: `share` (442); warm engines take K1B8W_GO2 with K1B_WARM_U for the attempt and the cold merge
      (450-455) and, on a window closed the plain way (425), the cold arm; K1B8_GO2 / K1B8W_GO2 fold the slots per thread (449, 462:
      >= 4 -> 4, == 2 -> 2, else 1); 463: narrow, k1b_u == 8 -> 8 else 4; 464: hist -> <4, true>, k1b_u == 8 -> <8, false>, else <4, false>.
    - k2_rowptr, lines 494-495: dh_g.  K4, do_layer, lines 562-572: split, use_mfma.  K5, do_score, lines 710-711: use_mfma."""
    k = dict(k1a_family=K1A_GLOBAL, k1a_l2=0, k1a_sharded=0, k1a_hist=0, k1a_nsub=0, k1a_pb=0,
             k1b_family=K1B_NONE, k1b_u=0, k1b_spt=0, k1b_pack=0, k1b_hist=0, k1b_share=0, k1b_warm=0,
             k2_dh=int(plan["dh_g"] != 0), k4_split=plan["k4_split"], k4_mfma=plan["use_mfma"], k5_mfma=plan["use_mfma"])
    if plan["variant"] != 0:
        return k
    k["k1a_sharded"] = int(world > 1)
    l2m = 2 if pa["l2_in_lds"] and pa["l2_u16"] else 1 if pa["l2_in_lds"] else 0
    if plan["narrow"] and pa["k1a_team"]:
        k.update(k1a_family=K1A_TEAM, k1a_l2=l2m, k1a_pb={256: 8, 512: 9}.get(plan["np"], 10))
    elif plan["narrow"]:
        k.update(k1a_family=K1A_TILE, k1a_l2=l2m, k1a_nsub=2 if pa["k1a_nsub"] == 2 else 1)
    else:
        k.update(k1a_family=K1A_WIDE, k1a_l2=int(bool(pa["l2_in_lds"])), k1a_hist=plan["hist"])
    k["k1b_share"] = int(plan["npb"] > cus and 2 * plan["k1b_lds"] <= LDS_BYTES)
    spt = plan["k1b_ht"] // plan["k1b_threads"]
    spt = 4 if spt >= 4 else 2 if spt == 2 else 1
    u = 8 if plan["k1b_u"] == 8 else 4
    if plan["warm"] or plan["narrow"]:
        k.update(k1b_family=K1B_STREAM, k1b_u=u, k1b_spt=spt, k1b_pack=plan["k1b_pack"], k1b_warm=plan["warm"])
    elif plan["hist"]:
        k.update(k1b_family=K1B_MERGE, k1b_u=4, k1b_hist=1)
    else:
        k.update(k1b_family=K1B_MERGE, k1b_u=u)
    return k


def choice_keys(k, warm_u):
    """(family of the library, template arguments) of every kernel an engine with this choice may launch"""
    keys = []
    if k["k1a_family"] == K1A_WIDE:
        keys.append(("k1a_wide", [k["k1a_l2"], k["k1a_sharded"], k["k1a_hist"]]))
    if k["k1a_family"] == K1A_TILE:
        keys.append(("k1a_tile", [k["k1a_l2"], k["k1a_sharded"], k["k1a_nsub"]]))
    if k["k1a_family"] == K1A_TEAM:
        keys.append(("k1a_team", [k["k1a_l2"], k["k1a_sharded"], k["k1a_pb"]]))
    if k["k1b_family"] == K1B_MERGE:
        keys.append(("k1b_merge", [k["k1b_u"], k["k1b_hist"], k["k1b_share"]]))
    if k["k1b_family"] == K1B_STREAM:
        keys.append(("k1b_stream", [k["k1b_u"], k["k1b_spt"], k["k1b_pack"], 0, k["k1b_share"]]))
        if k["k1b_warm"]:
            keys += [("k1b_stream", [warm_u, k["k1b_spt"], k["k1b_pack"], wm, k["k1b_share"]]) for wm in (1, 2)]
    keys += [("k4_layer", [fi, k["k4_mfma"], pj, k["k4_split"]]) for fi in (32, 64) for pj in (0, 1)]
    return keys


def test_kernel_choice_is_the_launch_ladders(plan_exe):
    """every case of plans.json (bench shapes, knob cases, the pass-A states after upserts): the planner's kernel choice against
    ladder_choice, and every kernel it may launch inside the instantiations the library enumerates"""
    cases = json.load(open(GOLDEN))["cases"]
    got = run_plans(plan_exe, [planner_input(c) for c in cases])
    domains, = plan_driver.run(plan_exe, (), args=("--domains",))
    warm_u = domains.pop("k1b_warm_u")
    # the instantiation counts of the library: k1b_merge and k1b_stream_merge each with a _wide twin
    assert {f: len(v) for f, v in domains.items()} == dict(k1a_wide=8, k1a_tile=12, k1a_team=18, k1b_merge=2 * 3, k1b_stream=2 * 24,
                                                           k4_layer=16)
    assert all(len(set(map(tuple, v))) == len(v) for v in domains.values())
    checked, families, after = 0, set(), 0
    for c in cases:
        have = got[c["name"]]
        if have["rc"] != 0:
            assert "kernels" not in have
            continue
        world = int(dict(t.split("=") for t in c["input"].split()).get("world", 1))
        for part, pa in (("kernels", "pass_a"), ("kernels_after", "pass_a_after")):
            if pa not in have:
                continue
            want = ladder_choice(have["plan"], have[pa], world, have["cus"])
            assert have[part] == want, (c["name"], part, {f: (want[f], have[part][f]) for f in want if want[f] != have[part].get(f)})
            for fam, key in choice_keys(have[part], warm_u):
                assert key in domains[fam], (c["name"], part, fam, key)
            checked += 1
            after += part == "kernels_after"
            families.add((have[part]["k1a_family"], have[part]["k1b_family"]))
    assert checked >= 127 + 11 and after >= 11
    # the recorded cases reach every pass-A and pass-B family
    assert families >= {(K1A_GLOBAL, K1B_NONE), (K1A_WIDE, K1B_MERGE), (K1A_TILE, K1B_STREAM), (K1A_TEAM, K1B_STREAM)}
