"""CPU tests of the node rollup (K9): the numpy reference tests/nodes_ref.py against a plain Python loop, NODE_DTYPE against the
header's sg_node_out, and the plan in alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage nodes) — memory and grids for every
window an engine can close."""
import os
import subprocess

import numpy as np

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.helpers import ref
from tests.nodes_ref import NO_ROW, key_score, nodes_loop, nodes_ref, score_key, score_q32
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def random_rows(seed, n, n_known=40, n_labels=6, n_obip=5):
    """rows in canonical order: every ref type, self-loops, alive-only rows, equal maximum scores, sums that wrap"""
    rng = np.random.default_rng(seed)
    refs = np.array([ref(0, v) for v in range(n_known)] + [ref(1, v) for v in range(n_labels)] + [ref(2, v) for v in range(n_obip)], np.uint32)
    pairs = set()
    while len(pairs) < n:
        f = refs[rng.integers(0, n_known)] if rng.random() < 0.8 else refs[rng.integers(0, len(refs))]
        pairs.add((int(f), int(refs[rng.integers(0, len(refs))])))
    pairs = sorted(pairs)                                             # (from, to) ascending: the canonical order
    r = np.zeros(n, dtype=EDGE_OUT_DTYPE)
    r["from_ref"] = [p[0] for p in pairs]
    r["to_ref"] = [p[1] for p in pairs]
    r["count"] = rng.integers(0, 1 << 20, n)
    r["count"][rng.random(n) < 0.15] = 0                              # alive-only rows
    r["err_count"] = np.minimum(r["count"], rng.integers(0, 1000, n))
    r["alive"] = rng.integers(0, 4, n)
    r["sum_ns"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(3)   # wraps when summed
    r["max_ns"] = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    r["sumsq_us"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    s = rng.choice(np.array([0.25, 0.5, 0.75, 0.9921875], np.float32), n)   # few values: many ties of the maximum
    s[::7] = rng.random(len(s[::7]), dtype=np.float32)
    s[::11] = 0.0
    r["score"] = s
    return r


def test_reference_equals_a_plain_loop():
    for seed in range(6):
        rows = random_rows(seed, 400)
        assert (rows["from_ref"] == rows["to_ref"]).sum() > 0 and (rows["count"] == 0).sum() > 0
        assert set(np.unique(rows["to_ref"] >> 30)) == {0, 1, 2}
        want = nodes_loop(rows)
        got = nodes_ref(rows)
        assert got.tobytes() == want.tobytes(), seed
    assert len(nodes_ref(rows[:0])) == 0 and len(nodes_loop(rows[:0])) == 0


def test_hand_computed_window():
    A, B, L, O = ref(0, 1), ref(0, 7), ref(1, 0), ref(2, 3)
    r = np.zeros(5, dtype=EDGE_OUT_DTYPE)
    r["from_ref"] = [A, A, A, B, B]
    r["to_ref"] = [A, B, L, B, O]                                     # two self-loops
    r["count"] = [2, 3, 0, 5, 1]
    r["err_count"] = [1, 0, 0, 2, 1]
    r["alive"] = [0, 1, 2, 0, 0]
    r["sum_ns"] = [10, 20, 0, (1 << 64) - 5, 9]
    r["max_ns"] = [7, 15, 0, 4, 9]
    r["score"] = np.array([0.5, 0.75, 0.75, 0.75, 0.25], np.float32)
    n = nodes_ref(r)
    assert list(n["ref"]) == [A, B, L, O]                             # KNOWN by id, then LABEL, then OBIP
    a, b, lab, ob = n
    assert (a["out_edges"], a["in_edges"], b["out_edges"], b["in_edges"]) == (3, 1, 2, 2)
    assert (a["out_count"], a["in_count"], b["in_count"]) == (5, 2, 8)
    assert b["out_sum_ns"] == ((1 << 64) - 5 + 9) % (1 << 64) and b["in_sum_ns"] == ((1 << 64) - 5 + 20) % (1 << 64)
    assert a["out_worst_row"] == 1 and a["out_score_max"] == np.float32(0.75)   # rows 1 and 2 tie: the smaller row
    assert b["in_worst_row"] == 1 and b["out_worst_row"] == 3
    assert a["in_worst_row"] == 0 and a["score"] == np.float32(0.75)
    assert lab["out_edges"] == 0 and lab["out_worst_row"] == NO_ROW and lab["out_score_max"] == 0 and lab["in_alive"] == 2
    assert ob["in_max_ns"] == 9 and ob["score"] == np.float32(0.25) and ob["in_err"] == 1
    assert a["out_score_q32"] == (1 << 31) + 3 * (1 << 30) + 3 * (1 << 30)


def test_score_keys_order_floats_and_round_trip():
    x = np.array([-1.0, -0.0, 0.0, 1e-30, 0.5, 1.0, np.inf], np.float32)
    k = score_key(x)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert key_score(k).tobytes() == x.tobytes()
    assert list(score_q32(np.array([-0.5, 0.0, 0.25, 1.0], np.float32))) == [0, 0, 1 << 30, 1 << 32]


def test_node_dtype_matches_the_header(tmp_path):
    fields = engine.NODE_DTYPE.names
    src = tmp_path / "node_layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "servicegraph.h"\nint main() {\n'
                   '    std::printf("size %zu\\n", sizeof(sg_node_out));\n'
                   + "".join(f'    std::printf("{f} %zu %zu\\n", offsetof(sg_node_out, {f}), sizeof(((sg_node_out*)0)->{f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "node_layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict((l.split()[0], tuple(int(x) for x in l.split()[1:])) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert out["size"] == (engine.NODE_DTYPE.itemsize,) == (136,)
    for f in fields:
        dt, off = engine.NODE_DTYPE.fields[f][:2]
        assert out[f] == (off, dt.itemsize), f


nodes_plan = plan_fixture("nodes")


def _around(*xs):
    return sorted({max(1, v + d) for x in xs for v in (x,) for d in (-1, 0, 1)})


EDGES = _around(1, 2048, 4096, 32768, 16 * 32768, 1 << 20) + [1_250_000, 1 << 24]
NCAPS = _around(1, 256, 2048, 4096, 256 * 1024, 256 * 1024 * 4) + [15_256, 1 << 22]


def test_plan_fits_every_window(nodes_plan):
    lines = [(me, 1000, s) for me in EDGES for s in (1, 2, 8)] + [(4096, nc, 1) for nc in NCAPS]
    for r in nodes_plan(lines):
        me, nc, T = r["max_edges"], r["ncap"], r["threads"]
        assert r["node_size"] == 136 and r["side_bytes"] == 64 and r["chunk"] == T * 8
        assert r["out_wgs"] * r["chunk"] >= me > (r["out_wgs"] - 1) * r["chunk"]          # every row in one chunk
        assert r["ranges"] * r["range_nodes"] >= nc > (r["ranges"] - 1) * r["range_nodes"]  # every node in one range
        assert 1 <= r["slices"] <= r["max_slices"]
        assert 1 <= r["node_wgs"] <= r["max_wgs"] and r["node_per"] % T == 0 and r["node_wgs"] * r["node_per"] >= nc
        assert (r["node_wgs"] - 1) * r["node_per"] < max(nc, 1)                          # no workgroup without nodes
        assert r["dst_bytes"] >= 4 * me and r["table_bytes"] >= 64 * nc and r["rows_bytes"] >= 136 * nc
        assert r["part_bytes"] >= r["ranges"] * r["slices"] * r["range_nodes"] * 64
        assert r["blk_bytes"] >= 2 * r["max_wgs"] * 4 and r["count_bytes"] >= 8 and r["lds_bytes"] == r["range_nodes"] * 64 <= 160 * 1024
        for k in ("dst_bytes", "table_bytes", "part_bytes", "blk_bytes", "rows_bytes", "count_bytes"):
            assert r[k] % 256 == 0
        assert r["total_bytes"] == r["dst_bytes"] + 2 * r["table_bytes"] + r["part_bytes"] + r["blk_bytes"] + r["slots"] * (r["rows_bytes"] + r["count_bytes"])
        check_layout(r, {"dst": 4 * me, "table_out": 64 * nc, "table_in": 64 * nc, "rows": 136 * nc, "blk": 2 * r["max_wgs"] * 4, "count": 8,
                         "part": r["ranges"] * r["slices"] * r["range_nodes"] * 64}, per_slot=("rows", "count"))


def test_plan_of_config3(nodes_plan):
    c3, = nodes_plan([(1_250_000, 15_000 + 128 + 128, 1)])
    assert (c3["out_wgs"], c3["ranges"], c3["slices"], c3["node_wgs"], c3["node_per"]) == (611, 8, 16, 60, 256)
    assert c3["part_bytes"] == 8 * 16 * 2048 * 64 and c3["total_bytes"] < 32 << 20
