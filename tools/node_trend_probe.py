"""K10 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the per-node baselines and the node selection cost per window.

One engine with the node rollup and the node trend on closes --windows windows; after each, the node rows are read whole
(window_nodes) and selected (window_nodes_top(k = 100), by score and by in_lat_dev), each timed on the host.  For the device time of
the K10 kernels run it under `rocprofv3 --kernel-trace --stats -- python tools/node_trend_probe.py --windows 3` (the k10_* and
k8_scan rows of the stats: this engine has no edge trend, so every k8_scan launch is K10's).  Prints one JSON line; --out also
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_nodes(); g.set_node_trend(warmup=1)
    nodes_ms, top_ms, top_dev_ms, ntr_ms = [], [], [], []
    n_nodes = 0
    for w in range(a.windows + 1):
        g.ingest_bulk(ev)
        g.flush_window_view()
        t0 = time.perf_counter()
        nodes = g.window_nodes()
        t1 = time.perf_counter()
        sel, idx, n_nodes = g.window_nodes_top(100)
        t2 = time.perf_counter()
        g.window_nodes_top(100, by="in_lat_dev")
        t3 = time.perf_counter()
        g.window_node_trend()
        t4 = time.perf_counter()
        assert len(nodes) == n_nodes and len(sel) == 100 and sel.tobytes() == nodes[idx].tobytes()
        if w == 0:                                                       # warm-up (the selection's scratch is allocated here)
            continue
        nodes_ms.append((t1 - t0) * 1e3); top_ms.append((t2 - t1) * 1e3); top_dev_ms.append((t3 - t2) * 1e3); ntr_ms.append((t4 - t3) * 1e3)
    s = g.node_trend_stats()
    med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
    res = {"config": 3, "nodes": int(n_nodes), "windows": a.windows, "entries": int(s.entries),
           "window_nodes_ms": med(nodes_ms), "window_nodes_top100_score_ms": med(top_ms),
           "window_nodes_top100_in_lat_dev_ms": med(top_dev_ms), "window_node_trend_ms": med(ntr_ms)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
