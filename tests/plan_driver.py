"""The CPU driver of alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp) for the plan tests: built once per pytest process, run
per stage.  A test module keeps its fixture's name and makes it here — rank_plan = plan_fixture("rank") for the window stages, whose
fixture is the runner; exe = stage_fixture("k5_form") for the engine-level stages, whose tests hand the fixture to run()."""
import json
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_built = None                               # (the directory's owner, the program's path)


def exe():
    global _built
    if _built is None:
        d = tempfile.TemporaryDirectory(prefix="plan_driver_")             # (removed when the process ends)
        path = os.path.join(d.name, "plan_driver")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", path, os.path.join(HERE, "micro", "plan_driver.cpp")])
        _built = (d, path)
    return _built[1]


def run_text(stage, lines=(), args=()):
    """what `plan_driver <stage> <args>` prints for these lines (a line: its text, or its fields); a zero exit status is asserted"""
    text = "".join((l if isinstance(l, str) else " ".join(map(str, l)) if isinstance(l, (tuple, list)) else str(l)) + "\n" for l in lines)
    out = subprocess.run([exe(), stage, *args], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def run(stage, lines, *, by_name=False, args=()):
    """the objects the stage prints, one per line — in order, or by their "name" """
    rows = [json.loads(l) for l in run_text(stage, lines, args).splitlines()]
    return {r["name"]: r for r in rows} if by_name else rows


def run_named(stage, lines):
    """run(), by name: the engine-level modules import it as their run(exe, lines)"""
    return run(stage, lines, by_name=True)


def plan_fixture(stage):
    """a module's fixture: lines -> the stage's objects"""
    @pytest.fixture(scope="module")
    def plan():
        exe()
        return lambda lines: run(stage, lines)
    return plan


def stage_fixture(stage):
    """a module's fixture: the stage, for run(fixture, lines), with the driver built"""
    @pytest.fixture(scope="module")
    def stage_name():
        exe()
        return stage
    return stage_name
