"""K11 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the culprit ranking costs per window.

Two engines of one configuration, both with the node rollup, one of them with the ranking on, close the same windows alternately
(A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the medians is the stage's cost on the
close path.  After each window of the ranking engine, window_rank_top(k = 10) is timed against window_nodes() + window_rank() of
every node.  For the device time per k11_* kernel run it under `rocprofv3 --kernel-trace --stats -- python tools/rank_probe.py
--windows 3 --only-on` (tools/gpu.sh run:...).  Prints one JSON line; --out also writes it to a file."""
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


def _engine(topo, ev, labels, L):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    g.set_nodes()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--only-on", action="store_true", help="the ranking engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L)
    on.set_rank(iters=a.iters)
    off = None if a.only_on else _engine(topo, ev, labels, L)
    t_on, t_off, top_ms, all_ms = [], [], [], []
    n_nodes = n_rows = 0
    for w in range(a.windows + 1):
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(ev)
            t0 = time.perf_counter()
            n_rows = len(g.flush_window_view())
            acc.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        sel, rk, idx, n_nodes = on.window_rank_top(10)
        t1 = time.perf_counter()
        nodes = on.window_nodes(); ranks = on.window_rank()
        t2 = time.perf_counter()
        assert len(nodes) == len(ranks) == n_nodes and len(sel) == 10 and sel.tobytes() == nodes[idx].tobytes() and rk.tobytes() == ranks[idx].tobytes()
        top_ms.append((t1 - t0) * 1e3); all_ms.append((t2 - t1) * 1e3)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    res = {"config": 3, "rows": int(n_rows), "nodes": int(n_nodes), "windows": a.windows, "iters": a.iters or 20,
           "flush_view_rank_on_ms": med(t_on), "window_rank_top10_ms": med(top_ms), "window_nodes_plus_rank_all_ms": med(all_ms),
           "top_share": float(rk["share"][0]), "mass": float(sum(int(x) for x in ranks["rank"]) / 2.0 ** 56)}
    if off is not None:
        res["flush_view_rollup_only_ms"] = med(t_off)
        res["rank_cost_ms"] = res["flush_view_rank_on_ms"]["median"] - res["flush_view_rollup_only_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
