"""K7 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what a selection costs and what it saves.

End to end, per window: sg_flush_window_top(k = 1000) against sg_flush_window_view, alternated on one engine (the window close
K1 pass B .. K5 is in both; the difference is the selection against the copy of every row).  For the device time of the selection
kernels run it under `rocprofv3 --kernel-trace --stats -- python tools/select_probe.py --windows 3` (the k7_* rows of the stats).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8, help="windows of each kind (alternated)")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=1_250_000, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    view_ms, top_ms, thr_ms = [], [], []
    n_edges = 0
    for w in range(2 * a.windows + 2):
        g.ingest_bulk(ev)
        t0 = time.perf_counter()
        if w < 2:                                                        # warm-up: one of each
            (g.flush_window_view() if w == 0 else g.flush_window_top(a.k))
            continue
        if w % 2 == 0:
            n_edges = len(g.flush_window_view()); view_ms.append((time.perf_counter() - t0) * 1e3)
        else:
            rows, idx, n = g.flush_window_top(a.k); top_ms.append((time.perf_counter() - t0) * 1e3)
            assert len(rows) == min(a.k, n) and n == n_edges
    # threshold mode selecting about 1 % of the rows
    g.ingest_bulk(ev)
    rows = g.flush_window_view().copy()
    t = float(np.quantile(rows["score"], 0.99))
    for _ in range(3):
        g.ingest_bulk(ev)
        t0 = time.perf_counter(); r, _, _ = g.flush_window_top(0, t); thr_ms.append((time.perf_counter() - t0) * 1e3)
    res = {"config": 3, "edges": n_edges, "k": a.k, "windows": a.windows,
           "flush_window_view_ms": {"median": float(np.median(view_ms)), "min": float(np.min(view_ms)), "max": float(np.max(view_ms))},
           "flush_window_top_ms": {"median": float(np.median(top_ms)), "min": float(np.min(top_ms)), "max": float(np.max(top_ms))},
           "flush_window_top_threshold_1pct_ms": {"median": float(np.median(thr_ms)), "rows": int(len(r))}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
