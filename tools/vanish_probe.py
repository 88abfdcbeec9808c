"""K8's vanished list and K7 by a trend key at BASELINE config 3 (1 M edges, 10 M events, L = 2): what they cost per window.

Two engines of the same config with the trend on, closing windows alternately; every other window pair drops one eighth of the
(saddr, daddr) pairs, so edges go silent and come back.  Engine A has the vanished list on and closes each window with
sg_flush_window_top_by(SG_SEL_LAT_DEV, k = 1000) (then reads its vanished list); engine B has the list off and closes each window
with sg_flush_window_view plus sg_window_trend of every row — what a caller does without the selection.  ms per window for each.
For the device time of the K8 kernels with the list on (k8_*_v) and off (k8_count / k8_scan / k8_write) and of k7_keys_by, run it
under `rocprofv3 --kernel-trace --stats -- python tools/vanish_probe.py --windows 3`.
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
    g.set_trend(warmup=1)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8, help="windows of each kind (alternated)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    group = ((ev["saddr"].astype(np.uint64) * 2654435761 + ev["daddr"].astype(np.uint64) * 40503) >> 7) % 8
    ev_drop = np.ascontiguousarray(ev[group != 3])
    A, B = _engine(topo, labels, L, len(ev)), _engine(topo, labels, L, len(ev))
    A.set_vanished()
    top_ms, view_ms, van_ms, vanished = [], [], [], []
    n_edges = 0
    for w in range(2 * a.windows + 4):
        g = A if w % 2 else B
        g.ingest_bulk(ev_drop if (w // 2) % 2 else ev)
        t0 = time.perf_counter()
        if g is A:
            sel, idx, n_edges = A.flush_window_top(1000, by="lat_dev")
            t1 = time.perf_counter()
            lst, n = A.window_vanished(with_count=True)
            t2 = time.perf_counter()
            assert len(sel) == 1000
        else:
            rows = B.flush_window_view()
            tr = B.window_trend()
            t1 = t2 = time.perf_counter()
            assert len(tr) == len(rows)
        if w < 4:                                                        # warm-up: two of each
            continue
        if g is A:
            top_ms.append((t1 - t0) * 1e3); van_ms.append((t2 - t1) * 1e3); vanished.append(int(n))
        else:
            view_ms.append((t1 - t0) * 1e3)
    med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
    res = {"config": 3, "edges": int(n_edges), "windows": a.windows, "entries": int(A.trend_stats().entries),
           "flush_window_top_by_lat_dev_k1000_ms": med(top_ms), "flush_window_view_plus_window_trend_ms": med(view_ms),
           "window_vanished_read_ms": med(van_ms), "vanished_per_window": vanished}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
