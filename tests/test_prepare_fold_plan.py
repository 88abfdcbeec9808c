"""Which window closes launch no kc_prepare (alaz_amd/csrc/sg_plan.hpp: Plan::prepare_fold for the engine, close_folds for one close),
on the CPU: tests/micro/plan_driver.cpp, stage prepare_fold, prints the choice for a config line.

The fold is for one shape only — a variant-0 narrow engine that keeps warm-window state, unsharded, whose pass B runs 1 024 threads —
and, per close, for the closes that launch the warm attempt (the close keeps state, the host tries the warm path) with the engine's
own outbound-IP collection (mode 1).  Everything else keeps the separate launch.  The engine reports Plan::prepare_fold as
geometry()["prepare_fold"] (sg_prepare_fold_get): tests/test_gpu_prepare_fold.py reads it there."""
from tests.plan_driver import run_named as run, stage_fixture

C3 = "max_known_nodes=15000 max_edges=1254096 layers=2 max_labels=64 max_window_events=10000000"     # the flagship shape
SMALL = "max_known_nodes=112 max_edges=2048 layers=1 max_labels=256 max_window_events=65536"           # the GPU test's shape


fold_exe = stage_fixture("prepare_fold")


# (name, config line, the plan folds, why)
CASES = [
    ("c3", C3, 1),
    ("c3_no_warm", f"{C3} flags=2", 0),                       # SG_CFG_NO_WARM: no kept state, no warm attempt to ride in
    ("c3_warm_knob_off", f"{C3} SG_WARM=0", 0),
    ("c3_sharded", f"{C3} world=2 rank=1", 0),                # the sharded closes pass union / gathered lists to kc_prepare
    ("c3_variant1", f"{C3} k1_variant=1", 0),                 # the global edge table: no pass B
    ("c3_wide_records", f"{C3} k1_variant=2", 0),             # 16-byte records keep no state
    ("c3_histogram", f"{C3} flags=1", 0),
    ("c3_512_threads", f"{C3} SG_K1B_THREADS=512", 0),        # the prepare workgroup strides by 1 024
    ("c3_u8", f"{C3} SG_K1B_U=8", 0),                         # the one-table-per-CU build has no warm instantiation
    ("c3_knob_off", f"{C3} SG_NO_FOLD=1", 0),
    ("c3_knob_zero", f"{C3} SG_NO_FOLD=0", 1),
    ("c3_no_order", f"{C3} SG_K1B_NO_ORDER=1", 1),            # the order is optional, the fold does not need it
    ("c3_two_slots", f"{C3} windows_in_flight=2", 1),
    ("small_auto", SMALL, 0),                                 # below 2^18 edges sg_create keeps no state by itself ...
    ("small_by_name", f"{SMALL} k1_variant=3 flags=4", 1),    # ... asked for by name (SG_CFG_WARM, the 8-byte path) it does
    ("small_twin", f"{SMALL} k1_variant=3 flags=4 SG_NO_FOLD=1", 0),
    ("small_ht256", f"{SMALL} k1_variant=3 flags=4 SG_NP=64 SG_HT=256", 1),   # pass B's smallest LDS still holds kc_prepare's scratch
]


def test_the_plan_folds_one_shape_only(fold_exe):
    got = run(fold_exe, [f"{n} {line}" for n, line, _ in CASES])
    for name, _, want in CASES:
        r = got[name]
        assert r["rc"] == 0, name
        assert r["prepare_fold"] == want, (name, r)
        if r["prepare_fold"]:
            assert r["warm"] == 1 and r["narrow"] == 1 and r["variant"] == 0 and r["k1b_threads"] == 1024, (name, r)
            assert r["k1b_lds"] >= r["prepare_lds"], (name, r)
    assert got["c3_512_threads"]["k1b_threads"] == 512 and got["c3_512_threads"]["warm"] == 1      # (only the thread count stands in the way)
    assert got["c3_sharded"]["warm"] == 1 and got["c3_knob_off"]["warm"] == 1


def test_a_close_folds_only_where_it_launches_the_warm_attempt(fold_exe):
    got = run(fold_exe, [f"{n} {line}" for n, line, _ in CASES])
    for name, _, folds in CASES:
        closes = {(w, t, ob): f for w, t, ob, f in got[name]["closes"]}
        assert len(closes) == 12
        for (warm, warm_try, ob_mode), f in closes.items():
            # plain-closed windows (warm 0), sg_set_warm(0) (warm_try 0), a caller's union list (mode 0), gathered lists (mode 2): kc_prepare
            assert f == int(bool(folds) and warm == 1 and warm_try == 1 and ob_mode == 1), (name, warm, warm_try, ob_mode)


def test_the_knob_is_the_development_builds(fold_exe):
    from alaz_amd import engine
    assert "SG_NO_FOLD" in engine.DEV_KNOBS
