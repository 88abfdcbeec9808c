"""K17 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the workload ranking and the selection over it cost.

Two engines of one configuration, both with the groups, the group trend (K15), the workload rows and their baseline (K16) on and
their pods in blocks of --block (20: a Deployment of 20 replicas), one of them with the workload ranking on (--iters iterations),
close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the
medians is the stage's cost on the close path.  After each window of the K17 engine, window_group_rank_top(k = --k) is timed against
window_groups() (every group edge, 80 bytes each, over PCIe, to walk on the host: the only way to a workload ranking without this
stage) and against window_group_rank() of every row.  The last window's rank rows are held to the reference (tests/group_rank_ref.py)
unless --no-check.  For the device time per kernel run it under `rocprofv3 --kernel-trace --stats -- python
tools/group_rank_probe.py --windows 3 --only-on --no-check` (the k17_* rows of the stats).  The stage's memory and its working
workgroups are the plan's to say (tests/micro/plan_driver.cpp, stage group_rank, prints plan_group_rank).  Prints one JSON line; --out also
writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alaz_amd import engine, replay, weights  # noqa: E402
from tests.helpers import CLOCK, HostShim  # noqa: E402

MAX_EDGES = 1_250_000


def _engine(topo, ev, labels, L, block):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=MAX_EDGES, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)            # a tight max_groups: the tables are per group key
    g.group_assign(pods, pods // block)
    g.set_group_trend(warmup=1)
    g.set_group_nodes(); g.set_group_node_trend(warmup=1)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=10, help="k of the timed selection")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-on", action="store_true", help="the K17 engine alone (profiler runs)")
    ap.add_argument("--no-check", action="store_true", help="skip the reference over the last window (slow in Python)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    on.set_group_rank(iters=a.iters)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, all_ms, rank_ms = [], [], [], [], []
    rng = np.random.default_rng(17)
    for w in range(a.windows + 1):
        e = ev.copy()                                                 # latency drifts, so that the windows are not all one
        e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.1 * w * rng.random(len(e)))).astype(np.uint64)
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(e)
            t0 = time.perf_counter()
            g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        top, rtop, idx, n_nodes = on.window_group_rank_top(a.k)
        top_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ge = on.window_groups()
        all_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rk = on.window_group_rank()
        rank_ms.append((time.perf_counter() - t0) * 1e3)
        assert n_nodes == len(rk) and rtop.tobytes() == rk[idx].tobytes()
    n = on.window_group_nodes()
    assert top.tobytes() == n[idx].tobytes()
    res = {"config": 3, "windows": a.windows, "block": a.block, "iters": a.iters, "group_edges": int(len(ge)), "workload_rows": int(len(n)),
           "groups": int((n["ref"] >> 30 == engine.REF_GROUP).sum()), "rank_sum_over_M": float(sum(int(x) for x in rk["rank"]) / (1 << 56)),
           "top_share": float(rtop["share"][0]) if len(rtop) else 0.0, "flush_view_k17_on_ms": med(t_on),
           f"window_group_rank_top{a.k}_ms": med(top_ms), "window_groups_all_ms": med(all_ms), "window_group_rank_all_ms": med(rank_ms),
           "group_edge_bytes": int(ge.nbytes), "rank_row_bytes": int(rk.nbytes)}
    if not a.no_check:
        from tests.group_rank_ref import group_rank_ref
        t0 = time.perf_counter()
        want = group_rank_ref(ge, n, iters=a.iters)
        res["reference_s"] = time.perf_counter() - t0
        res["equals_reference"] = bool(want.tobytes() == rk.tobytes())
    if off is not None:
        res["flush_view_k17_off_ms"] = med(t_off)
        res["k17_cost_ms"] = res["flush_view_k17_on_ms"]["median"] - res["flush_view_k17_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
