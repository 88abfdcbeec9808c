"""K15 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the workload baselines and the selection over group edges cost.

Two engines of one configuration, both with the groups on and their pods in blocks of --block (20: a Deployment of 20 replicas),
one of them with the group trend on, close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host
for each, and the difference of the medians is the stage's cost on the close path.  After each window of the K15 engine,
window_groups_top(k = --k, by lat_dev) is timed against window_groups() (every group edge, 80 bytes each, over PCIe), and
window_group_trend() once.  For the device time per kernel run it under
`rocprofv3 --kernel-trace --stats -- python tools/group_trend_probe.py --windows 3 --only-on` (the k15_* rows of the stats and
k8_scan: this engine has no edge or node trend, so every k8_scan launch is K15's).
The stage's memory is the plan's to say (tests/micro/plan_driver.cpp, stage group_trend, prints plan_group_trend, plan_vanished and
plan_group_select for a max_edges).  Prints one JSON line; --out also writes it to a file."""
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
    g.set_groups()
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.group_assign(pods, pods // block)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=1000, help="k of the timed selection")
    ap.add_argument("--only-on", action="store_true", help="the K15 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    on.set_group_trend(warmup=1); on.set_group_vanished()
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, all_ms, trend_ms = [], [], [], [], []
    rng = np.random.default_rng(15)
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
        top, idx, n_groups = on.window_groups_top(a.k, by="lat_dev")
        top_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ge = on.window_groups()
        all_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        tr = on.window_group_trend()
        trend_ms.append((time.perf_counter() - t0) * 1e3)
        assert n_groups == len(ge) == len(tr) and top.tobytes() == ge[idx].tobytes()
    s = on.group_trend_stats()
    res = {"config": 3, "windows": a.windows, "block": a.block, "group_edges": int(len(ge)), "entries": int(s.entries),
           "rows_with_lat_dev": int((tr["lat_dev"] != 0).sum()), "flush_view_k15_on_ms": med(t_on),
           f"window_groups_top{a.k}_lat_dev_ms": med(top_ms), "window_groups_all_ms": med(all_ms), "window_group_trend_ms": med(trend_ms)}
    if off is not None:
        res["flush_view_k15_off_ms"] = med(t_off)
        res["k15_cost_ms"] = res["flush_view_k15_on_ms"]["median"] - res["flush_view_k15_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
