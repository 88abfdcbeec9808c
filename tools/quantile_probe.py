"""K20 at BASELINE config 3 (1 M edges, 10 M events, L = 2) with the edge histogram on: what the latency percentiles cost.

Two engines of one configuration, both with the node rollup (K9), the groups (K14) and the workload rows (K16) on and their pods in
blocks of --block, one of them with sg_set_quantiles over --spaces, close the same windows alternately (A B A B ...):
sg_flush_window_view is timed on the host for each, and the difference of the medians is the stage's cost on the close path.  After
each window of the K20 engine the p99 of --k workloads (window_group_node_quantiles with an index) is timed against the only way to
them without this stage: window_hist() plus the rows already in hand.  For the device time per kernel run it under
`rocprofv3 --kernel-trace --stats -- python tools/quantile_probe.py --windows 3 --only-on` (the k20_* rows of the stats).  The
stage's memory is the plan's to say (tests/micro/plan_driver.cpp, stage quantile, prints plan_quantiles).  Prints one JSON line; --out also
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
                            max_window_events=len(ev), edge_histogram=True)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.set_nodes()
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)
    g.group_assign(pods, pods // block)
    g.set_group_nodes()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=100, help="workloads whose p99 is read")
    ap.add_argument("--spaces", default="nodes,groups,group_nodes")
    ap.add_argument("--only-on", action="store_true", help="the K20 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    spaces = tuple(a.spaces.split(","))
    on.set_quantiles(spaces)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, p99_ms, hist_ms = [], [], [], []
    rng = np.random.default_rng(20)
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
            gn = on.window_group_nodes()
            idx = rng.integers(0, len(gn), a.k).astype(np.uint32)
            t0 = time.perf_counter()
            q = on.window_group_node_quantiles(idx)
            p99_ms.append((time.perf_counter() - t0) * 1e3)
            assert q.shape == (a.k, 2, 2)
        t0 = time.perf_counter()
        h = on.window_hist()
        hist_ms.append((time.perf_counter() - t0) * 1e3)
    res = {"config": 3, "windows": a.windows, "block": a.block, "spaces": list(spaces), "rows": int(n_rows), "hist_bytes": int(h.nbytes),
           "flush_view_k20_on_ms": med(t_on), "window_hist_all_ms": med(hist_ms)}
    if p99_ms:
        res[f"workload_p99_of_{a.k}_ms"] = med(p99_ms)
        res["workload_rows"] = int(len(gn))
    if "groups" in spaces:
        res["group_edges"] = int(len(on.window_groups()))
    if "nodes" in spaces:
        res["nodes"] = int(len(on.window_nodes()))
    if off is not None:
        res["flush_view_k20_off_ms"] = med(t_off)
        res["k20_cost_ms"] = res["flush_view_k20_on_ms"]["median"] - res["flush_view_k20_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
