"""K23 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the traffic baselines cost.

Two engines of one configuration, both with the node rollup (K9), the groups (K14), the workload rows (K16) and the four mean
baselines (K8, K10, K15, K16's) on, their pods in blocks of --block, one of them with sg_set_traffic_trend over --spaces, close the
same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the medians is
the stage's cost on the close path.  After each window of the K23 engine the question the stage answers — the --k workloads whose
inbound traffic fell furthest (window_group_nodes_top_traffic, "drop" of the "in" side) — is timed against the only way to it
without this stage: every workload row of the window (window_group_nodes), the history kept on the host.  The same selections by
the mean baselines' rows run beside them (window_nodes_top, window_groups_top, window_group_nodes_top), so that one profiler run
has k23_keys next to k10_keys / k15_keys over the same rows.  For the device time per kernel run it under `rocprofv3
--kernel-trace --stats -- python tools/traffic_probe.py --windows 3 --only-on`: the k23_* rows of the stats beside k8_count /
k8_write, k10_count / k10_write, k15_count / k15_write and k16_tcount / k16_twrite of the same run, the mean baselines of the same
spaces on the same inputs.  The stage's memory is the plan's to say (tests/micro/plan_driver.cpp, stage traffic_trend, prints
plan_traffic_trend).  Prints one JSON line; --out also writes it to a file."""
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
    g.set_nodes()
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)
    g.group_assign(pods, pods // block)
    g.set_group_nodes()
    g.set_trend(); g.set_node_trend(); g.set_group_trend(); g.set_group_node_trend()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=20, help="workloads selected by their drop of inbound traffic")
    ap.add_argument("--spaces", default="edges,nodes,groups,group_nodes")
    ap.add_argument("--only-on", action="store_true", help="the K23 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    spaces = tuple(a.spaces.split(","))
    on.set_traffic_trend(spaces)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, all_ms = [], [], [], []
    rng = np.random.default_rng(23)
    for w in range(a.windows + 1):
        e = ev[rng.random(len(ev)) < 1.0 - 0.03 * w]                  # the traffic thins out from window to window
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(e)
            t0 = time.perf_counter()
            rows = g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)
        n_rows = len(rows)
        if "group_nodes" in spaces:
            t0 = time.perf_counter()
            sel, idx, n_wl = on.window_group_nodes_top_traffic(a.k, by="drop", side="in")
            top_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            every = on.window_group_nodes()
            all_ms.append((time.perf_counter() - t0) * 1e3)
            assert len(every) == n_wl and len(sel) <= a.k
            on.window_group_nodes_top(a.k, by="in_lat_dev")           # k10_keys over the same rows
        if "nodes" in spaces:
            on.window_nodes_top_traffic(a.k, by="drop", side="in"); on.window_nodes_top(a.k, by="in_lat_dev")
        if "groups" in spaces:
            on.window_groups_top_traffic(a.k, by="drop"); on.window_groups_top(a.k, by="lat_dev")   # k15_keys over the same rows
    res = {"config": 3, "windows": a.windows, "block": a.block, "spaces": list(spaces), "rows": int(n_rows),
           "flush_view_k23_on_ms": med(t_on)}
    for s in spaces:
        st = on.traffic_trend_stats(s)
        res[f"{s}_entries"] = int(st.entries); res[f"{s}_dropped"] = int(st.dropped)
    if top_ms:
        res[f"top_{a.k}_workloads_by_drop_ms"] = med(top_ms)
        res["every_workload_row_ms"] = med(all_ms)
        res["workload_rows"] = int(n_wl)
    if off is not None:
        res["flush_view_k23_off_ms"] = med(t_off)
        res["k23_cost_ms"] = res["flush_view_k23_on_ms"]["median"] - res["flush_view_k23_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
