"""K19 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the workload tracks cost.

Two engines of one configuration, both with K14 - K18 on (the groups, the group trend, the workload rows and their baseline, the
workload ranking and the workload incidents) and their pods in blocks of --block (20: a Deployment of 20 replicas), one of them with
the workload tracks on, close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the
difference of the medians is the stage's cost on the close path.  Two phases of --windows windows each: the threshold at the 0.99
quantile of a window's own score_max ("p99"), and every group edge red ("all": min_value = -inf).  After each window of the K19
engine, window_group_incident_tracks() is timed against window_groups() (every group edge, 80 bytes each, over PCIe, to walk and
match components on the host: the only way to workload tracks without K18 and this stage).  The last window's rows of each phase are
held to the reference (tests/group_track_ref.py, fed every window of the phase) unless --no-check.  For the device time per kernel
run it under `rocprofv3 --kernel-trace --stats -- python tools/group_track_probe.py --windows 3 --only-on --no-check` (the k13_* and
k19_* rows of the stats; K13 itself is off here, so the k13_* rows are this stage's).  The stage's memory is the plan's to say
(tests/micro/plan_driver.cpp, stage group_track, prints plan_group_tracks).  Prints one JSON line; --out also writes it to a file."""
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
INF = float("inf")


def _engine(topo, ev, labels, L, block, iters):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=MAX_EDGES, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev))
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)            # a tight max_groups: the tables are per group key
    g.group_assign(pods, pods // block)
    g.set_group_trend(warmup=1)
    g.set_group_nodes(); g.set_group_node_trend(warmup=1)
    g.set_group_rank(iters=iters)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--iters", type=int, default=20, help="K17's iterations, on both engines")
    ap.add_argument("--quiet", type=int, default=2, help="quiet_windows")
    ap.add_argument("--only-on", action="store_true", help="the K19 engine alone (profiler runs)")
    ap.add_argument("--no-check", action="store_true", help="skip the reference (slow in Python)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block, a.iters)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block, a.iters)
    med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
    rng = np.random.default_rng(19)
    res = {"config": 3, "windows": a.windows, "block": a.block, "iters": a.iters, "quiet_windows": a.quiet}
    w = 0

    def close(timed):
        nonlocal w
        e = ev.copy()                                                 # latency drifts, so that the windows are not all one
        e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.1 * w * rng.random(len(e)))).astype(np.uint64)
        w += 1
        for g, acc in ((on, timed[0]), (off, timed[1])):
            if g is None:
                continue
            g.ingest_bulk(e)
            t0 = time.perf_counter()
            g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)

    for g in (on, off):
        if g is not None:
            g.set_group_incidents(by="score", min_value=INF)
    close(([], []))                                                   # warm-up, and the window whose score_max sets the p99 threshold
    v = on.window_groups()["score_max"]
    p99 = float(np.sort(v[~np.isnan(v)])[int(0.99 * (len(v) - 1))])
    for phase, thr in (("p99", p99), ("all", -INF)):
        for g in (on, off):
            if g is not None:
                g.set_group_incidents(by="score", min_value=thr)
        on.set_group_tracks(quiet_windows=a.quiet)                    # (every sg_set_group_incidents call switched it off)
        ref = None
        if not a.no_check:
            from tests.group_track_ref import GroupTrackRef
            ref = GroupTrackRef(a.quiet, 0, ncap=len(on.window_group_nodes()) + 1)   # (never cut: any capacity above the rows does)
        want = None

        def follow():
            nonlocal want
            if ref is not None:
                want = ref.step(on.window_group_nodes(), on.window_group_node_incident(), on.window_group_incidents())
        close(([], []))                                               # (the first close after the switch is left out of the timing)
        follow()
        t_on, t_off, trk_ms, all_ms = [], [], [], []
        for _ in range(a.windows):
            close((t_on, t_off))
            t0 = time.perf_counter()
            trk = on.window_group_incident_tracks()
            trk_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ge = on.window_groups()
            all_ms.append((time.perf_counter() - t0) * 1e3)
            follow()
        st = on.group_track_stats()
        ended = on.window_group_tracks_ended()
        r = {"min_value": thr, "group_edges": int(len(ge)), "workload_rows": int(len(on.window_group_nodes())), "incidents": int(len(trk)),
             "continued": int(((trk["flags"] & engine.TRACK_NEW) == 0).sum()), "ended": int(len(ended)), "live_tracks": int(st.live),
             "opened": int(st.opened), "flush_view_k19_on_ms": med(t_on), "window_group_incident_tracks_ms": med(trk_ms),
             "window_groups_all_ms": med(all_ms), "group_edge_bytes": int(ge.nbytes), "track_bytes": int(trk.nbytes)}
        if ref is not None:
            r["equals_reference"] = bool(want[0].tobytes() == trk.tobytes() and want[1].tobytes() == ended.tobytes()
                                         and ref.entries().tobytes() == on.group_track_entries().tobytes())
        if off is not None:
            r["flush_view_k19_off_ms"] = med(t_off)
            r["k19_cost_ms"] = r["flush_view_k19_on_ms"]["median"] - r["flush_view_k19_off_ms"]["median"]
        res[phase] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
