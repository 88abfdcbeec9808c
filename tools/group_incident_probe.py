"""K18 at BASELINE config 3 (1 M edges, 10 M events, L = 2): what the workload incidents cost.

Two engines of one configuration, both with the groups, the group trend (K15), the workload rows and their baseline (K16) and the
workload ranking (K17) on and their pods in blocks of --block (20: a Deployment of 20 replicas), one of them with the workload
incidents on, close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the
difference of the medians is the stage's cost on the close path.  Two phases of --windows windows each: the threshold at the 0.99
quantile of a window's own score_max ("p99"), and every group edge red ("all": min_value = -inf).  After each window of the K18
engine, window_group_incidents() is timed against window_groups() (every group edge, 80 bytes each, over PCIe, to walk components
on the host: the only way to workload incidents without this stage).  The last window's incidents of each phase are held to the
reference (tests/group_incident_ref.py) unless --no-check.  For the device time per kernel run it under `rocprofv3 --kernel-trace
--stats -- python tools/group_incident_probe.py --windows 3 --only-on --no-check` (the k18_* rows of the stats).  The stage's memory
is the plan's to say (tests/micro/plan_driver.cpp, stage group_incident, prints plan_group_incidents).  Prints one JSON line; --out also
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
    ap.add_argument("--only-on", action="store_true", help="the K18 engine alone (profiler runs)")
    ap.add_argument("--no-check", action="store_true", help="skip the reference over the last window of each phase (slow in Python)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block, a.iters)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block, a.iters)
    med = lambda x: {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}   # noqa: E731
    rng = np.random.default_rng(17)
    res = {"config": 3, "windows": a.windows, "block": a.block, "iters": a.iters}
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

    on.set_group_incidents(by="score", min_value=INF)
    close(([], []))                                                   # warm-up, and the window whose score_max sets the p99 threshold
    v = on.window_groups()["score_max"]
    p99 = float(np.sort(v[~np.isnan(v)])[int(0.99 * (len(v) - 1))])
    for phase, thr in (("p99", p99), ("all", -INF)):
        on.set_group_incidents(by="score", min_value=thr)
        close(([], []))                                               # (the first close after the switch allocates nothing, but is left out)
        t_on, t_off, inc_ms, all_ms = [], [], [], []
        for _ in range(a.windows):
            close((t_on, t_off))
            t0 = time.perf_counter()
            inc = on.window_group_incidents()
            inc_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ge = on.window_groups()
            all_ms.append((time.perf_counter() - t0) * 1e3)
        n = on.window_group_nodes()
        r = {"min_value": thr, "group_edges": int(len(ge)), "workload_rows": int(len(n)), "incidents": int(len(inc)),
             "red_group_edges": int(inc["edges"].sum()), "largest_incident_rows": int(inc["nodes"].max()) if len(inc) else 0,
             "flush_view_k18_on_ms": med(t_on), "window_group_incidents_ms": med(inc_ms), "window_groups_all_ms": med(all_ms),
             "group_edge_bytes": int(ge.nbytes), "incident_bytes": int(inc.nbytes)}
        if not a.no_check:
            from tests.group_incident_ref import group_incident_ref
            t0 = time.perf_counter()
            want, winc = group_incident_ref(ge, n, "score", thr, rank=on.window_group_rank())
            r["reference_s"] = time.perf_counter() - t0
            r["equals_reference"] = bool(want.tobytes() == inc.tobytes() and winc.tobytes() == on.window_group_node_incident().tobytes())
        if off is not None:
            r["flush_view_k18_off_ms"] = med(t_off)
            r["k18_cost_ms"] = r["flush_view_k18_on_ms"]["median"] - r["flush_view_k18_off_ms"]["median"]
        res[phase] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
