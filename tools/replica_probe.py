"""K25 at BASELINE config 3 (1 M edges, 10 M events, 2 model layers) with the edge histogram on: what the replica outliers cost.

Two engines of one configuration, both with the node rollup (K9), the groups (K14), the workload rows (K16) and the latency
percentiles (K20) over the node rows on, their pods in blocks of --block, one of them with sg_set_replicas (tails at --permille, 0:
off), close the same windows alternately (A B A B ...): sg_flush_window_view is timed on the host for each, and the difference of the
medians is the stage's cost on the close path.  After each window of the K25 engine the question the stage answers — the --k replicas
furthest above their peers' error rate (window_replicas_top) — is timed against the only way to it without this stage: every node
row, every workload row and every node histogram to the host (window_nodes, window_group_nodes, window_node_hist), the group map
kept there.  For the device time per kernel run it under `rocprofv3 --kernel-trace --stats -- python tools/replica_probe.py --windows 3
--only-on`: the k25_* rows of the stats (and k20_pos_groups, which the stage launches once more a window) beside K9's and K16's
rollups (k9_out, k9_in_part, k16_out, k16_in_part) of the same run.  The stage's memory is the plan's to say
(tests/micro/replica_plan_test.cpp prints plan_replicas).  Prints one JSON line; --out also writes it to a file."""
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


def _engine(topo, ev, labels, L, block):
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=MAX_EDGES, layers=L, max_labels=128, max_outbound_ips=128,
                            max_window_events=len(ev), edge_histogram=True)
    g.set_clock(*CLOCK); g.load_weights(weights.make_weights(L))
    HostShim().apply(g, topo.k8s_ops()); g.set_label_count(len(labels))
    pods = np.arange(topo.n_pods, dtype=np.uint32)                    # node ids 0 .. P-1 are the pods (Topology.k8s_ops)
    g.set_nodes()
    g.set_groups(max_groups=int(topo.n_pods // block) + 1)
    g.group_assign(pods, pods // block)
    g.set_group_nodes()
    g.set_quantiles(("nodes",))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--block", type=int, default=20, help="pods per group")
    ap.add_argument("--k", type=int, default=20, help="replicas selected by their error excess")
    ap.add_argument("--permille", type=int, default=990, help="the tails' percentile, 0: no tails")
    ap.add_argument("--only-on", action="store_true", help="the K25 engine alone (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    topo, ev, labels, L = replay.make_config(3)
    on = _engine(topo, ev, labels, L, a.block)
    off = None if a.only_on else _engine(topo, ev, labels, L, a.block)
    on.set_replicas(tail_permille=a.permille)
    med = lambda x: {"median": float(np.median(x[1:])), "min": float(np.min(x[1:])), "max": float(np.max(x[1:]))}   # noqa: E731  (window 0: warm-up)
    t_on, t_off, top_ms, all_ms = [], [], [], []
    rng = np.random.default_rng(25)
    tally = dict(members=0, judged=0, outliers=0)
    for w in range(a.windows + 1):
        e = ev.copy()
        e["duration_ns"] = (e["duration_ns"].astype(np.float64) * (1.0 + 0.1 * w * rng.random(len(e)))).astype(np.uint64)
        for g, acc in ((on, t_on), (off, t_off)):
            if g is None:
                continue
            g.ingest_bulk(e)
            t0 = time.perf_counter()
            rows = g.flush_window_view()
            acc.append((time.perf_counter() - t0) * 1e3)
        n_rows = len(rows)
        t0 = time.perf_counter()
        sel, idx, n_nodes = on.window_replicas_top(a.k, 1, by="err", side="in")
        top_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        nodes, wl, h = on.window_nodes(), on.window_group_nodes(), on.window_node_hist()
        all_ms.append((time.perf_counter() - t0) * 1e3)
        assert len(nodes) == len(h) == n_nodes and len(sel) <= a.k
        groups = on.window_group_replicas()
        tally = dict(members=int((on.window_replicas()[:, 0] != 0xFFFFFFFF).sum()), judged=int(groups[:, 1].sum() + groups[:, 5].sum()),
                     outliers=int(groups[:, 2].sum() + groups[:, 6].sum()))
    res = {"config": 3, "windows": a.windows, "block": a.block, "tail_permille": a.permille, "rows": int(n_rows), "node_rows": int(n_nodes),
           "workload_rows": int(len(wl)), "last_window": tally, "flush_view_k25_on_ms": med(t_on),
           f"top_{a.k}_replicas_by_error_excess_ms": med(top_ms), "every_node_row_workload_row_and_histogram_ms": med(all_ms), "selected": int(len(sel))}
    if off is not None:
        res["flush_view_k25_off_ms"] = med(t_off)
        res["k25_cost_ms"] = res["flush_view_k25_on_ms"]["median"] - res["flush_view_k25_off_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
