"""The engine's launch plan (alaz_amd/csrc/sg_plan.hpp) on the CPU: tests/micro/plan_test.cpp prints the plan of every case of
tests/golden/plans.json, which holds the sizing decisions the engine made at commit 38499a0 — before the planner existed —
recorded on an MI355X from that commit's own sg_create, with and without the development build's SG_* overrides."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plans.json")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), os.path.join(HERE, "micro", "plan_test.cpp")])
    return str(exe)


def run_plans(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return {r["name"]: r for r in map(json.loads, out.stdout.splitlines())}


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


def test_knob_list_is_the_engines(plan_exe):
    from alaz_amd import engine
    out = subprocess.run([plan_exe, "--knobs"], capture_output=True, text=True, timeout=60, check=True)
    assert tuple(out.stdout.split()) == engine.DEV_KNOBS
