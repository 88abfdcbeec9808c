"""bench.py's two kinds of run: a plain one (the headline figure only) and --full (every leg beside it)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "scaling", "vs_baseline",
            "data", "config", "value_basis"}
FULL_ONLY = {"roofline", "kernels", "per_step", "box", "warm_windows", "effective_sclk_mhz", "settle", "end_to_end", "cpu_baseline",
             "overlapped", "value_end_to_end"}


def test_plain_is_the_default_and_full_is_asked_for():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.config) == (False, 7, 2, 3)
    assert bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"]).full
    with pytest.raises(SystemExit) as ex:
        bench.parse(["--help"])
    assert ex.value.code == 0


def test_stream_is_a_leg_of_the_full_run():
    with pytest.raises(SystemExit):
        bench.parse(["--config", "5", "--stream"])
    assert bench.parse(["--config", "5", "--stream", "--full"]).stream


def test_headline_fields():
    a = bench.parse(["--steps", "10", "--warmup", "1"])
    topo = SimpleNamespace(n_svcs=5, edge_src=[0] * 40)
    geo = {"k1_variant": 0, "k1_narrow": 1, "partitions": 256}
    res = bench.headline(a, 3, {"pods": 10}, topo, 1000, 2, 2, geo, 0.5)
    assert set(res) == HEADLINE
    assert res["value"] == pytest.approx(1000 * 10 / 0.5) and res["ms_per_step"] == pytest.approx(50.0)
    assert (res["unit"], res["higher_is_better"], res["dtype"]) == ("events/s", True, "u64")
    assert res["config"]["events_per_window"] == 1000 and "40 edges" in res["config"]["workload"]
    json.dumps(res)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps(engine_lib, tmp_path):
    out = tmp_path / "rows"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--batches", "2", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert set(res) == HEADLINE | {"dump_outputs"} and not set(res) & FULL_ONLY
    assert res["value"] > 0 and res["ms_per_step"] > 0 and (res["steps"], res["warmup"]) == (3, 1)
    d = res["dump_outputs"]
    assert d["rows"] > 0 and all((out / f).is_file() for f in d["files"])
