"""K8 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the per-edge baselines cost per window.

Two engines of the same config, one with the trend on and one with it off, closing windows alternately (sg_flush_window_view, the
trend rows of the window read back on the trend engine); ms per window for each.  For the device time of the K8 kernels run it
under `rocprofv3 --kernel-trace --stats -- python tools/trend_probe.py --windows 3` (the k8_* rows of the stats).
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


def _engine(topo, labels, L, n_ev):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=n_ev)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8, help="windows of each kind (alternated)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on, off = _engine(topo, labels, L, len(ev)), _engine(topo, labels, L, len(ev))
    on.set_trend()
    on_ms, off_ms, trend_ms = [], [], []
    n_edges = 0
    for w in range(2 * a.windows + 2):
        g = on if w % 2 else off
        g.ingest_bulk(ev)
        t0 = time.perf_counter()
        n_edges = len(g.flush_window_view())
        t1 = time.perf_counter()
        if g is on:
            tr = on.window_trend()
            assert len(tr) == n_edges
            trend_ms.append((time.perf_counter() - t1) * 1e3)
        if w < 2:                                                        # warm-up: one of each
            continue
        (on_ms if g is on else off_ms).append((t1 - t0) * 1e3)
    s = on.trend_stats()
    med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
    res = {"config": 3, "edges": n_edges, "windows": a.windows, "entries": int(s.entries),
           "flush_window_view_trend_on_ms": med(on_ms), "flush_window_view_trend_off_ms": med(off_ms),
           "trend_on_minus_off_ms": float(np.median(on_ms) - np.median(off_ms)),
           "window_trend_read_ms": med(trend_ms)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
