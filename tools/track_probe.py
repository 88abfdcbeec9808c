"""K13 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what following a window's incidents across windows costs.

Two engines of one configuration, both with the node rollup and the incidents on, one of them with the tracks on, close the same
windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the medians is the
stage's cost on the close path.  Twice: with every row red (min_value = -inf: one incident that holds every node, so every node
folds into one incident word) and with the threshold at the window's 99th score percentile (many small incidents, a table of as
many tracks).  After each window of the tracks engine, window_incident_tracks() + window_tracks_ended() is timed.  For the device
time per k13_* kernel run it under `rocprofv3 --kernel-trace --stats -- python tools/track_probe.py --windows 3 --only-on`.
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
    g.set_nodes()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--quiet-windows", type=int, default=2)
    ap.add_argument("--only-on", action="store_true", help="the tracks engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L)
    off = None if a.only_on else _engine(topo, ev, labels, L)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    res = {"config": 3, "windows": a.windows, "quiet_windows": a.quiet_windows}
    thr = float("-inf")
    for case in ("all_red", "p99"):
        for g in (on, off):
            if g is not None:
                g.set_incidents(min_value=thr)
        on.set_tracks(quiet_windows=a.quiet_windows)
        t_on, t_off, read_ms = [], [], []
        for w in range(a.windows + 1):
            for g, acc in ((on, t_on), (off, t_off)):
                if g is None:
                    continue
                g.ingest_bulk(ev)
                t0 = time.perf_counter()
                rows = g.flush_window_view()
                acc.append((time.perf_counter() - t0) * 1e3)
                if g is on and w == 0:
                    score = rows["score"].copy()
            t0 = time.perf_counter()
            tracks = on.window_incident_tracks(); ended = on.window_tracks_ended()
            read_ms.append((time.perf_counter() - t0) * 1e3)
        inc = on.window_incidents()
        st = on.track_stats()
        # the same events every time: the incidents should continue their tracks (continued == incidents, nothing ended or opened late)
        assert len(tracks) == len(inc) and st.windows == a.windows + 1 and len(set(tracks["track"].tolist())) == len(tracks)
        r = {"min_value": thr, "rows": int(len(score)), "nodes": int(len(on.window_node_incident())), "incidents": int(len(inc)),
             "largest_incident_nodes": int(inc["nodes"].max()) if len(inc) else 0, "tracks_live": int(st.live), "tracks_opened": int(st.opened),
             "continued_last_window": int((tracks["flags"] & engine.TRACK_NEW == 0).sum()), "ended_last_window": int(len(ended)),
             "flush_view_tracks_on_ms": med(t_on), "read_tracks_ms": med(read_ms)}
        if off is not None:
            r["flush_view_incidents_only_ms"] = med(t_off)
            r["track_cost_ms"] = r["flush_view_tracks_on_ms"]["median"] - r["flush_view_incidents_only_ms"]["median"]
        res[case] = r
        thr = float(np.sort(score)[int(0.99 * (len(score) - 1))])      # the 99th percentile of the window's scores
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
