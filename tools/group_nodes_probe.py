"""K16 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the workload rows, their baseline and the selection over them cost.

Two engines of one configuration, both with the groups and the group trend (K15) on and their pods in blocks of --block (20: a
Deployment of 20 replicas), one of them with the workload rows and their baseline on, close the same windows alternately (A B A B
...): sg_flush_window_view is timed on the host for each, and the difference of the medians is the stage's cost on the close path.
After each window of the K16 engine, window_group_nodes_top(k = --k) is timed against window_groups() (every group edge, 80 bytes
each, over PCIe: the only way to workload rows without this stage) and against window_group_nodes().  For the device time per
kernel run it under `rocprofv3 --kernel-trace --stats -- python tools/group_nodes_probe.py --windows 3 --only-on` (the k16_* rows
of the stats).  The stage's memory is the plan's to say (tests/micro/plan_driver.cpp, stage group_nodes, prints plan_group_nodes,
plan_group_node_trend and plan_group_node_select).  Prints one JSON line; --out also writes it to a file."""
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
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=100, help="k of the timed selection")
    ap.add_argument("--only-on", action="store_true", help="the K16 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    on.set_group_nodes(); on.set_group_node_trend(warmup=1)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, top_dev_ms, all_ms, nodes_ms = [], [], [], [], [], []
    rng = np.random.default_rng(16)
    for w in range(a.windows + 1):
        e = ev.copy()                                                 # latency drifts, so that the deviations are not all zero
        e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.1 * w * rng.random(len(e)))).astype(np.uint64)
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(e)
            t0 = time.perf_counter()
            g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        top, idx, n_nodes = on.window_group_nodes_top(a.k)
        top_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        on.window_group_nodes_top(a.k, by="in_lat_dev")
        top_dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ge = on.window_groups()
        all_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        n = on.window_group_nodes()
        nodes_ms.append((time.perf_counter() - t0) * 1e3)
        assert n_nodes == len(n) and top.tobytes() == n[idx].tobytes()
    tr = on.window_group_node_trend()
    s = on.group_node_trend_stats()
    res = {"config": 3, "windows": a.windows, "block": a.block, "group_edges": int(len(ge)), "workload_rows": int(len(n)),
           "groups": int((n["ref"] >> 30 == engine.REF_GROUP).sum()), "entries": int(s.entries),
           "rows_with_in_lat_dev": int((tr["in_lat_dev"] != 0).sum()), "flush_view_k16_on_ms": med(t_on),
           f"window_group_nodes_top{a.k}_score_ms": med(top_ms), f"window_group_nodes_top{a.k}_in_lat_dev_ms": med(top_dev_ms),
           "window_groups_all_ms": med(all_ms), "window_group_nodes_all_ms": med(nodes_ms),
           "group_edge_bytes": int(ge.nbytes), "workload_row_bytes": int(n.nbytes)}
    if off is not None:
        res["flush_view_k16_off_ms"] = med(t_off)
        res["k16_cost_ms"] = res["flush_view_k16_on_ms"]["median"] - res["flush_view_k16_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
