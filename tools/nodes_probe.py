"""K9 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the node rollup costs per window.

Two engines of the same config, one with the rollup on and one with it off, closing windows alternately (sg_flush_window_view, the
node rows of the window read back on the rollup engine); ms per window for each.  For the device time of the K9 kernels run it
under `rocprofv3 --kernel-trace --stats -- python tools/nodes_probe.py --windows 3` (the k9_* rows of the stats), or pass
--stats <kernel_stats.csv> to fold such a file into the result line.
Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alaz_amd import engine, replay, weights  # noqa: E402
from tests.helpers import CLOCK, HostShim  # noqa: E402


def _engine(topo, labels, L, n_ev):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=n_ev)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def k9_stats(path: str) -> dict:
    """the k9_* rows of a rocprofv3 kernel_stats.csv: calls, average and total device time (us)"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if not name.startswith("k9_"):
                continue
            k = name.split("(")[0]
            out[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "total_us": float(r["TotalDurationNs"]) / 1e3}
    if out:
        out["per_window_us"] = sum(v["avg_us"] for v in out.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8, help="windows of each kind (alternated)")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv of a run of this tool: its k9_* rows")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.stats:
        res = {"config": 3, "k9_device": k9_stats(a.stats)}
    else:
        topo, ev, labels, L = replay.make_config(3)
        on, off = _engine(topo, labels, L, len(ev)), _engine(topo, labels, L, len(ev))
        on.set_nodes()
        on_ms, off_ms, read_ms = [], [], []
        n_edges = n_nodes = 0
        for w in range(2 * a.windows + 2):
            g = on if w % 2 else off
            g.ingest_bulk(ev)
            t0 = time.perf_counter()
            n_edges = len(g.flush_window_view())
            t1 = time.perf_counter()
            if g is on:
                n_nodes = len(on.window_nodes())
                read_ms.append((time.perf_counter() - t1) * 1e3)
            if w < 2:                                                    # warm-up: one of each
                continue
            (on_ms if g is on else off_ms).append((t1 - t0) * 1e3)
        med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
        res = {"config": 3, "edges": n_edges, "nodes": n_nodes, "windows": a.windows,
               "flush_window_view_nodes_on_ms": med(on_ms), "flush_window_view_nodes_off_ms": med(off_ms),
               "nodes_on_minus_off_ms": float(np.median(on_ms) - np.median(off_ms)), "window_nodes_read_ms": med(read_ms)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
