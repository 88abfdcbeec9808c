"""K24 at BASELINE config 3 (1 M edges, 10 M events, 2 model layers) with the edge histogram on: what the SLO burn rates cost.

Two engines of one configuration, both with the node rollup (K9), the groups (K14), the workload rows (K16), the latency
percentiles (K20) over the two node-shaped spaces and the node and workload mean baselines (K10, K16's: the yardstick of the
device time) on, their pods in blocks of --block, one of them with sg_set_slo over --spaces and --long windows, close the same
windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the medians is the
stage's cost on the close path.  After each window of the K24 engine the question the stage answers — the --k workloads burning
their error budget fastest (window_group_nodes_top_slo) — is timed against the only way to it without this stage: every workload
row and every workload histogram to the host (window_group_nodes, window_group_node_hist), the history kept there.  For the device
time per kernel run it under `rocprofv3 --kernel-trace --stats -- python tools/slo_probe.py --windows 3 --only-on`: the k24_* rows of
the stats beside k10_count / k10_write and k16_tcount / k16_twrite of the same run.  The stage's memory is the plan's to say
(tests/micro/slo_plan_test.cpp prints plan_slo).  Prints one JSON line; --out also writes it to a file."""
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
NODE_SPACES = ("nodes", "group_nodes")


def _engine(topo, ev, labels, L, block):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=MAX_EDGES, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev), edge_histogram=True)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.set_nodes()
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)
    g.group_assign(pods, pods // block)
    g.set_group_nodes()
    g.set_quantiles(NODE_SPACES)
    g.set_node_trend(); g.set_group_node_trend()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=20, help="workloads selected by their error burn")
    ap.add_argument("--spaces", default="nodes,group_nodes")
    ap.add_argument("--short", type=int, default=2)
    ap.add_argument("--long", type=int, default=64)
    ap.add_argument("--only-on", action="store_true", help="the K24 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    spaces = tuple(a.spaces.split(","))
    on.set_slo(spaces, short_windows=a.short, long_windows=a.long, min_burn_q10=1024)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, all_ms = [], [], [], []
    rng = np.random.default_rng(24)
    for w in range(a.windows + 1):
        e = ev.copy()
        e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.1 * w * rng.random(len(e)))).astype(np.uint64)
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
            sel, idx, n_wl = on.window_group_nodes_top_slo(a.k, 1024, by="err", side="in")
            top_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            wl, h = on.window_group_nodes(), on.window_group_node_hist()
            all_ms.append((time.perf_counter() - t0) * 1e3)
            assert len(wl) == len(h) == n_wl and len(sel) <= a.k
    res = {"config": 3, "windows": a.windows, "block": a.block, "spaces": list(spaces), "short": a.short, "long": a.long, "rows": int(n_rows),
           "flush_view_k24_on_ms": med(t_on)}
    for s in spaces:
        st = on.slo_stats(s)
        res[f"{s}_keys"] = int(st.keys); res[f"{s}_keys_active"] = int(st.keys_active); res[f"{s}_sides_burning"] = int(st.sides_burning)
    if top_ms:
        res[f"top_{a.k}_workloads_by_error_burn_ms"] = med(top_ms)
        res["every_workload_row_and_histogram_ms"] = med(all_ms)
        res["workload_rows"] = int(n_wl); res["selected"] = int(len(sel))
    if off is not None:
        res["flush_view_k24_off_ms"] = med(t_off)
        res["k24_cost_ms"] = res["flush_view_k24_on_ms"]["median"] - res["flush_view_k24_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
