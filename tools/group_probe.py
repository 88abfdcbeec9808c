"""K14 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what contracting a window's service map to workloads costs.

Two engines of one configuration, one of them with the groups on and its pods in blocks of --block (20: a Deployment of 20
replicas), close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference
of the medians is the stage's cost on the close path.  After each window of the groups engine, window_groups() is timed (80 bytes
per group edge cross PCIe).  For the device time per k14_* kernel run it under
`rocprofv3 --kernel-trace --stats -- python tools/group_probe.py --windows 3 --only-on`.
Prints one JSON line; --out also writes it to a file."""
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
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--only-on", action="store_true", help="the groups engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L)
    off = None if a.only_on else _engine(topo, ev, labels, L)
    on.set_groups()
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    on.group_assign(pods, pods // a.block)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, read_ms = [], [], []
    for w in range(a.windows + 1):
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(ev)
            t0 = time.perf_counter()
            rows = g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)
            if g is on:
                n_rows, count = len(rows), int(rows["count"].sum())
        t0 = time.perf_counter()
        ge = on.window_groups()
        read_ms.append((time.perf_counter() - t0) * 1e3)
    assert int(ge["edges"].sum()) == n_rows and int(ge["count"].sum()) == count      # every row is in exactly one group edge
    res = {"config": 3, "windows": a.windows, "block": a.block, "rows": n_rows, "group_edges": int(len(ge)),
           "largest_group_edge_rows": int(ge["edges"].max()), "flush_view_groups_on_ms": med(t_on), "read_groups_ms": med(read_ms)}
    if off is not None:
        res["flush_view_groups_off_ms"] = med(t_off)
        res["group_cost_ms"] = res["flush_view_groups_on_ms"]["median"] - res["flush_view_groups_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
