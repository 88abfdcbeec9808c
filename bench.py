#!/usr/bin/env python3
"""bench.py — L7 edge-events/s ingested -> scored service map on MI355X (BASELINE.json metric).

A step = one window of the hot path over one batch of synthetic events that is already resident in HBM ("device-resident
replay"): K1 resolve_aggregate over the batch, then K2..K5 (CSR build, node/edge features, SAGE layers, edge scores) and
the window reset.  Workloads (BASELINE.json configs, alaz_amd/replay.py):

  --gpus 1 (default)  C3: 10k pods / 5k services / 1M edges (power-law), 10M HTTP events per window, 2 SAGE layers —
                      the largest single-GPU configuration.  --config 2 (1k pods / 50k edges / 1M events, 1 layer) and
                      --config 5 (100k pods / 20M edges, 5M mixed HTTP/Kafka/Postgres events per window, on ONE GPU)
                      are selectable.
  --gpus N > 1        C4: C3's graph hash-sharded by source pod over the N GPUs (alaz_amd/sharded.py); `value` = STRONG scaling
                      (the same 10M-event replay routed over the N GPUs), the weak figure (10M events per GPU and window) in `weak`.

Steps cycle through a ring of distinct batches larger than the 256 MiB Infinity Cache, so every step streams its events
from HBM.  One JSON line on stdout (rank 0).  A plain one-GPU run sets up, settles, warms up, times the steps, writes
--dump-outputs if asked and prints the headline fields (metric, value, unit, higher_is_better, dtype, ms_per_step, the
workload); everything below beside `value` is measured only with --full, which runs every leg the line has:

  value        events/s of the timed device-resident steps (never includes PCIe; `end_to_end` does)
  roofline     the dominant kernel K1 (pass A k1a_team_partition + pass B k1b_stream_merge): algorithmic bytes 32*Ev + 32*E per window
                / their dispatch durations (HIP events on the launch stream), vs 8 TB/s
  per_step     median / min / p90 / max of >= 100 single windows (SURVEY 8(d) run protocol); box: dependent-load latencies of this box
  warm_windows the engine keeps the union of the edges its windows touched: value is the steady state of a replay whose
               windows touch edges it has seen; cold_ms_per_step = the same steps with every window rebuilt from nothing
  kernels      the same for every kernel group of the window (K1a, K1b, K2, K3-in, K3-feat, K4, K5)
  end_to_end   events accepted by sg_ingest from HOST memory (several feeder threads, pinned staging ring, H2D) until the
               window's rows are back in host memory (sg_flush_window): SURVEY §8(d)(i); bounded by PCIe (32 B/event in)
  cpu_baseline the reference's CPU path restated in C (oracle/, the Go aggregator cannot be built here), timed on this
               box's host cores on a bounded sample of the same workload
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
F_IN, F_HID = 32, 64
DUMP_MAX_ROWS = 1 << 19      # --dump-outputs: 10 float64 + 3 float32 fields = 92 B a row, 48 MiB at most
DUMP_SEED = 0xA1A2D0           # --dump-outputs: the hash that picks the sample


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="timed windows (0 = per config: C2 200, C3/C4 30, C5 10)")
    ap.add_argument("--warmup", type=int, default=-1, help="untimed windows (-1 = per config: C2 20, C3/C4 5, C5 2)")
    ap.add_argument("--config", type=int, default=0, choices=[0, 2, 3, 4, 5], help="0 = 3 for one GPU, 4 (C3's graph sharded) for several")
    ap.add_argument("--batches", type=int, default=0, help="distinct event batches in the HBM ring (0 = auto)")
    ap.add_argument("--full", action="store_true", help="one GPU: also measure everything beside the headline figure — "
                                                       "CPU baseline, per-step distribution, K1 roofline, per-kernel groups, cold path, churn, "
                                                       "several windows in flight, end-to-end from host memory, box probes (the --no-* options "
                                                       "below leave single legs out).  Without it a run does only what `value` needs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-end-to-end", action="store_true", help="--full: skip the end-to-end pass")
    ap.add_argument("--no-churn", action="store_true", help="--full: skip the churn leg (windows that bring 0.1 %% / 1 %% / 4 %% new edges)")
    ap.add_argument("--stream", action="store_true", help="--full, config 5 only: add the streaming run (tools/c5_stream.py: raw 1096-byte records at the "
                                                         "nominal 5 M events/s through the C++ host side, a window per second, ten windows)")
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="--full: seconds per CPU-baseline variant")
    ap.add_argument("--feeders", type=int, default=8, help="--full: host threads calling sg_ingest in the end-to-end pass")
    ap.add_argument("--windows", type=int, default=1, help="window slots in flight for the timed region (sg_config.windows_in_flight); "
                                                            "1 keeps the per-kernel timings uncontended")
    ap.add_argument("--overlap-windows", type=int, default=4, help="--full: extra diagnostic pass with this many windows in flight (0 = skip)")
    ap.add_argument("--graph", choices=["fixed", "scaled"], default="fixed",
                    help="N > 1: 'fixed' shards the configuration's own graph over the N GPUs (what BASELINE's multi-GPU configurations "
                         "do with theirs); 'scaled' also grows the graph N-fold")
    ap.add_argument("--shard-of", type=int, default=1, help="one GPU: time ONE shard of the configuration hash-sharded over this many GPUs (BASELINE config 5 is "
                                                              "specified for 8): the shard's sub-graph (edges whose source pod it owns) with every IP replicated, "
                                                              "its routed share of every window's events, in an engine sized for the shard — the shape a rank of "
                                                              "the 8-GPU job has, without the exchanges")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N > 1, which mode `value` is: 'strong' (default) = ONE replay, the same Ev-event windows routed over the N GPUs by the "
                         "owner of each event's source (BASELINE config 4: total work fixed); 'weak' = Ev events per GPU and window (the event "
                         "volume grows with N).  The other mode is run briefly too and reported in the line's `weak` / `strong` object")
    ap.add_argument("--verify", action="store_true", help="N > 1 (or SG_FORCE_SHARDED): one untimed window of a global trace through the sharded engines, rows "
                                                            "gathered on rank 0 and compared byte for byte with an unsharded engine -> rows_verified in the line")
    ap.add_argument("--settle-ms", type=float, default=400.0, help="untimed real windows run for at least this long before the warm-up steps, so that the "
                                                                   "GPU's power management has left its idle state when the clock starts (0 = none)")
    ap.add_argument("--profile-mode", action="store_true", help="only warm-up + the timed steps (no diagnostic passes, no CPU baseline): "
                                                                  "the run rocprofv3 wraps, so its per-kernel averages are those of the timed region")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the edge rows the last timed window produced (what sg_window_read hands a caller) as "
                         "DIR/<field>.npy, one file per sg_edge_out field, ordered by (from_ref, to_ref); float64, the fp32 fields float32; "
                         f"above {DUMP_MAX_ROWS} rows a fixed seeded sample of that many edges.  One GPU, one window in flight")
    a = ap.parse_args(argv)
    if a.dump_outputs and (a.gpus > 1 or a.windows > 1):
        ap.error("--dump-outputs reads the last timed window back with sg_window_read: --gpus 1 and --windows 1 only")
    if a.stream and not a.full:
        ap.error("--stream is one of the --full legs: add --full")
    if a.config == 0:
        a.config = 3 if a.gpus == 1 else 4
    dflt = {2: (200, 20), 3: (30, 5), 4: (30, 5), 5: (10, 2)}[a.config]
    if a.steps <= 0:
        a.steps = dflt[0]
    if a.warmup < 0:
        a.warmup = dflt[1]
    return a


# ------------------------------------------------------------------------------------------------
# CPU baseline (oracle/ = measurement infrastructure; runs BEFORE the GPU runtime is initialised so that
# the multi-process variant can fork)
# ------------------------------------------------------------------------------------------------
def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


_W = {}


def _faithful_worker(secs):
    """child process: one oracle instance, the faithful string path on the shared (copy-on-write) sample"""
    from oracle import pyoracle
    o = pyoracle.Oracle(1_000_000_000, 1_700_000_000_000_000_000)
    o.apply_ops(_W["ops"])
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < secs:
        o.l7_wire(_W["wire"]); done += _W["n"]
    dt = time.perf_counter() - t0
    o.close()
    return done, dt


def _lean_worker(secs):
    from oracle import pyoracle
    topo, ev = _W["topo"], _W["ev"]
    l = pyoracle.Lean(topo.n_nodes, 2 * min(len(topo.edge_src), len(ev)) + 1024)     # (sized by what the sample can touch: a C5-sized table per process exhausted a box)
    for i in range(topo.n_pods):
        l.upsert_pod(int(topo.pod_ips[i]), i)
    for j in range(topo.n_svcs):
        l.upsert_service(int(topo.svc_ips[j]), topo.n_pods + j)
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < secs:
        l.reset_window(); l.process(ev); done += len(ev)
    dt = time.perf_counter() - t0
    l.close()
    return done, dt


def cpu_baseline(topo, events, labels, layers, seconds):
    """The reference's CPU path restated, every figure in events/s on this box's host cores:
      faithful_1t  oracle/sg_oracle.c on full 1096-byte l7_event records: processL7 -> processHttpEvent -> setFromToV2 ->
                   PersistRequest with dotted-quad strings and string-keyed tables, one heap row per request — what the Go
                   aggregator does per event (aggregator/data.go:1208-1249, 827-870; datastore/backend.go:819-847), 1 thread
      faithful_Nt  the same in one PROCESS per host core (independent tables: an upper bound for the lock-sharing original)
      lean_1t/_Nt  oracle/lean_baseline.c: the same join + per-edge aggregation on u32 keys and open-addressing tables over
                   packed 32-byte events — what a careful CPU implementation of K1 would do
      scoring_1t   the window close (CSR, features, SAGE layers, scores — builder-defined, the reference has none) of the
                   sample's graph, events of the sample / close time
    `value` = faithful_1t (kind "port": a C restatement; the Go binary cannot be built here: no Go toolchain)."""
    import multiprocessing as mp
    from alaz_amd import replay, weights
    from oracle import pyoracle
    pyoracle.build()
    n_f = min(len(events), 200_000)
    sample = events[:n_f]
    wire = replay.to_wire(sample, labels)
    lean_ev = np.ascontiguousarray(events[: min(len(events), 2_000_000)])
    _W.update(ops=topo.k8s_ops(), wire=wire, n=n_f, topo=topo, ev=lean_ev)
    res = {"unit": "events/s", "kind": "port", "cpu_model": _cpu_model(), "host_cpus": os.cpu_count()}
    # 1 thread, in this process
    d, dt = _faithful_worker(seconds)
    res["faithful_1t"] = d / dt
    d, dt = _lean_worker(max(2.0, seconds / 2))
    res["lean_1t"] = d / dt
    # the window close on the sample's graph
    o = pyoracle.Oracle(1_000_000_000, 1_700_000_000_000_000_000)
    o.apply_ops(_W["ops"]); o.packed(sample, labels)
    t0 = time.perf_counter(); o.window_close(weights.make_weights(layers), layers); tc = time.perf_counter() - t0
    res["scoring_1t"] = n_f / tc
    res["scoring_1t_note"] = f"window close of the {n_f}-event sample's graph ({len(o.edge_dict())} edges) in {tc * 1e3:.0f} ms"
    o.close()
    nc = max(1, min(os.cpu_count() or 1, 128))
    try:                                                             # never more processes than a quarter of the free memory carries
        avail = next(int(ln.split()[1]) * 1024 for ln in open("/proc/meminfo") if ln.startswith("MemAvailable"))
        ent = 2 * (2 * min(len(topo.edge_src), len(lean_ev)) + 1024) + 16                  # oracle/lean_baseline.c: next power of two of this
        per_proc = (256 << 20) + 48 * (1 << (ent - 1).bit_length()) + 600 * topo.n_nodes + 2 * len(wire)
        nc = max(1, min(nc, int(0.25 * avail / per_proc)))
        if len(topo.edge_src) > 5_000_000: nc = min(nc, 32)          # C5: the forked children also share a multi-GB topology copy-on-write
    except Exception:
        nc = min(nc, 16)
    if nc > 1:
        ctx = mp.get_context("fork")
        for name, fn, secs in (("faithful_Nt", _faithful_worker, max(3.0, seconds / 2)), ("lean_Nt", _lean_worker, max(2.0, seconds / 3))):
            with ctx.Pool(nc) as pool:
                t0 = time.perf_counter()
                outs = pool.map(fn, [secs] * nc)
                wall = time.perf_counter() - t0
            res[name] = sum(x[0] / x[1] for x in outs)                 # sum of per-process rates over the same interval
            res[name + "_procs"] = nc
            res[name + "_wall_s"] = round(wall, 1)
    res["value"] = res["faithful_1t"]; res["cores"] = 1
    res["sample"] = (f"{n_f} events of the same workload as full 1096-B l7_event records (faithful), {len(lean_ev)} packed events (lean), each "
                     f"repeated for ~{seconds:.0f} s; C restatement of processL7..PersistRequest (oracle/sg_oracle.c) — the Go aggregator itself "
                     "cannot be built here (no Go toolchain)")
    return res


def kernel_src_sha():
    """Hash of the kernel sources (the same function as tools/pmc_k1_json.py): names the build the counters were taken on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "alaz_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip", ".hpp")):
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(config):
    """HBM bytes per K1 window from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs of
    `bench.py --profile-mode`, `tools/gpu.sh pmc:TAG:CONFIG`; gfx950 corrections per MI355X_MICROARCH.md are applied by
    tools/pmc_k1_json.py).  Counters cannot be read from inside the process being timed, so this is the last committed
    measurement for this workload (traffic_measured_in_run: false), or null.  The third value says whether the counters
    were taken on the kernel sources this run is timing."""
    path = os.path.join(ROOT, "profiles", f"pmc_k1_c{config}.json")
    try:
        with open(path) as f:
            j = json.load(f)
        src = f"profiles/pmc_k1_c{config}.json ({j.get('round', '?')}, git {j.get('git_head', '?')})"
        return float(j["k1_total_hbm_bytes"]), src, j.get("kernel_src_sha") == kernel_src_sha(), j.get("k1_total_hbm_bytes_calibrated")
    except Exception:
        return None, None, None, None


def measured_copy_gbs(torch):
    """Device-to-device copy rate of this box (read + write bytes / time), SURVEY.md 8(d)."""
    n = 1 << 30
    x = torch.empty(n, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
    y.copy_(x); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        y.copy_(x)
    e1.record(); torch.cuda.synchronize()
    return 2.0 * n * 5 / (e0.elapsed_time(e1) * 1e-3) / 1e9


def dump_outputs(path, rows, obips):
    """--dump-outputs: the rows of one window as DIR/<field>.npy, ordered by (from_ref, to_ref) so that two builds compare row for
    row whatever order they emit.  A window of more than DUMP_MAX_ROWS edges is sampled by a seeded hash of (from_ref, to_ref): the
    same edges are picked whenever they are there.  edges_in_window.npy holds the full row count; outbound_ips.npy, the table that
    resolves OBIP refs, only when the window has raw outbound destinations (an HTTP-only replay has none: no empty file is written).
    Returns what was written."""
    os.makedirs(path, exist_ok=True)
    key = (rows["from_ref"].astype(np.uint64) << np.uint64(32)) | rows["to_ref"].astype(np.uint64)
    n_all = len(rows)
    if n_all > DUMP_MAX_ROWS:
        with np.errstate(over="ignore"):                     # murmur3 fmix64 (a bijection: one row per edge, so no ties)
            h = key ^ np.uint64(DUMP_SEED)
            h = (h ^ (h >> np.uint64(33))) * np.uint64(0xFF51AFD7ED558CCD)
            h = (h ^ (h >> np.uint64(33))) * np.uint64(0xC4CEB9FE1A85EC53)
            h ^= h >> np.uint64(33)
        pick = np.argpartition(h, DUMP_MAX_ROWS - 1)[:DUMP_MAX_ROWS]
        rows, key = rows[pick], key[pick]
    rows = rows[np.argsort(key, kind="stable")]
    files = {}
    for name in rows.dtype.names:
        col = rows[name]
        files[name] = col.astype(np.float32 if col.dtype.kind == "f" else np.float64)    # (the u64 sums of a window stay far below 2^53)
    if len(obips):
        files["outbound_ips"] = np.asarray(obips).astype(np.float64)
    files["edges_in_window"] = np.array([n_all], dtype=np.float64)
    for name, arr in files.items():
        np.save(os.path.join(path, f"{name}.npy"), arr)
    return {"dir": path, "rows": int(len(rows)), "edges_in_window": n_all, "sampled": n_all > DUMP_MAX_ROWS,
            "bytes": int(sum(arr.nbytes for arr in files.values())), "files": sorted(f"{k}.npy" for k in files)}


def algorithmic_bytes(Ev, E, N, L):
    """compulsory traffic per window and kernel group."""
    b = {"K1a": 32.0 * Ev, "K1b": 32.0 * E, "K2": 16.0 * E + 4.0 * (N + 1), "K3-in": 32.0 * E, "K3-feat": 4.0 * F_IN * N,
         "K5": 52.0 * E + 2 * 4.0 * F_HID * N}
    k4 = 0.0
    for l in range(L):
        k4 += 4.0 * (N + 1) + 4.0 * E + 4.0 * (F_IN if l == 0 else F_HID) * N + 4.0 * F_HID * N
    b["K4"] = k4
    return b


def self_launch(a):
    """`python bench.py --gpus N` without a launcher: check that the node has N GPUs, then re-run this script under
    torch.distributed.run (one process per GPU over RCCL) and pass rank 0's JSON line through.  Failures come out as ONE JSON
    object with an "error" field and a non-zero exit code, never as a traceback."""
    import socket
    import subprocess

    def fail(msg, **kw):
        print(json.dumps({"metric": "L7 edge-events/s ingested->scored service-map", "value": None, "unit": "events/s", "n_gpus": a.gpus,
                          "error": msg, **kw}), flush=True)
        return 2
    try:
        probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=300)
        have = int(probe.stdout.strip().splitlines()[-1])
    except Exception as ex:                                          # noqa: BLE001
        return fail(f"could not count GPUs: {ex}")
    if have < a.gpus:
        return fail(f"--gpus {a.gpus} needs {a.gpus} visible GPUs, this node has {have}", gpus_visible=have)
    with socket.socket() as sk:                                      # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)     # (stderr passes through)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        return fail(f"torch.distributed.run exited with {out.returncode}", stdout_tail=out.stdout[-400:])
    print(lines[-1], flush=True)
    return 0


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(a)                                        # `python bench.py --gpus N`: one rank per GPU under torch.distributed.run
    force_sharded = os.environ.get("SG_FORCE_SHARDED") == "1"      # exercise the multi-GPU code path at world = 1
    if a.dump_outputs and (world > 1 or force_sharded):
        sys.exit("bench.py: --dump-outputs reads the last timed window back from the unsharded engine: not with the sharded path")
    # the contract is ONE line on stdout: libraries that print there (RCCL writes its version banner to stdout when the
    # first communicator is created) are sent to stderr for the duration of the run
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    try:
        if world > 1 or force_sharded:
            import torch
            import torch.distributed as dist
            from alaz_amd import sharded
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            try:
                res = sharded.bench(a, rank, world, local)
            except Exception as ex:                                  # noqa: BLE001
                # one line saying what failed, on the real stdout, then the exception itself: a rank that exits non-zero makes
                # torch.distributed.run end the others (they may be waiting for it in a collective)
                os.write(saved_stdout, (json.dumps({"metric": "L7 edge-events/s ingested->scored service-map", "value": None, "unit": "events/s",
                                                    "n_gpus": world, "rank": rank, "error": repr(ex)[:400]}) + "\n").encode())
                raise
        else:
            res = bench_single(a, local)
    finally:
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        os.close(saved_stdout)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1 or force_sharded:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def headline(a, cfgno, c, topo, Ev, L, nb, geo, dt):
    """The fields every one-GPU line has (all that a plain run prints): the figure of the timed steps and the workload it was taken on."""
    variant = ("global-table K1 (variant 1)" if geo["k1_variant"] == 1 else
               f"partitioned K1 (variant 0, {'8' if geo['k1_narrow'] else '16'}-byte records, {geo['partitions']} partitions)")
    return {
        "metric": "L7 edge-events/s ingested->scored service-map", "value": Ev * a.steps / dt, "unit": "events/s",
        "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        # (one GPU: the job of the N > 1 default — BASELINE config 4 = this replay routed over N ranks, total work fixed — at N = 1)
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u64", "data": "synthetic",
        "config": {"workload": (f"ONE SHARD OF {a.shard_of} of " if a.shard_of > 1 else "") + f"C{cfgno} device-resident replay: {c['pods']} pods / {topo.n_svcs} services / {len(topo.edge_src)} edges, "
                               f"{Ev} {'mixed HTTP/Kafka/Postgres' if cfgno == 5 else 'HTTP'} l7 events per window already in HBM, {L}-layer SAGE + MLP score, "
                               f"{variant}; {nb}-batch HBM ring (value excludes PCIe: see end_to_end with --full)",
                   "events_per_window": Ev, "layers": L, "windows_in_flight": a.windows, "shard_of": a.shard_of,
                   "parallelism": "1 GPU" if a.shard_of == 1 else f"1 GPU standing in for one rank of {a.shard_of} (no exchanges: K1 and the local window close of the shard's shape)"},
        "value_basis": "mean over the timed steps (wall clock around K back-to-back windows, one window in flight)",
    }


def geo_warm(g) -> bool:
    """does this engine carry the edge set from window to window (sg_geometry.warm_windows)"""
    try:
        return bool(g.geometry().get("warm_windows", 0))
    except Exception:                                        # noqa: BLE001
        return False


def _engine_for(a, topo, labels, c, device, windows, engine, weights):
    L = c["layers"]
    big = a.config == 5
    # edge capacity: the graph's edges (a shard view holds its own only), but never more than a window has events — a window cannot touch
    # more distinct edges than it has events, and the partition count / table sizes follow the capacity (config 5: 20 M edges in the graph,
    # 5 M events per window: the partitioned K1 instead of the global-table variant; SG_BENCH_FULL_EDGE_CAP=1 sizes for the whole graph)
    n_edges = len(topo.edge_src)
    if not os.environ.get("SG_BENCH_FULL_EDGE_CAP"):
        n_edges = min(n_edges, max(1, c["events"] // a.shard_of))
    g = engine.ServiceGraph(max_known_nodes=topo.n_nodes, max_edges=int(n_edges * (1.1 if big and a.shard_of == 1 else 1.25)) + 4096, layers=L,
                            max_labels=max(64, len(labels)), max_outbound_ips=64, device=device, max_batch=int(os.environ.get("SG_BENCH_MAX_BATCH", 1 << 20)),
                            max_window_events=max(1, c["events"] // a.shard_of), windows_in_flight=windows,
                            # config 5's Kafka / Postgres requests to outside addresses are raw outbound IPs in every window: no window can close warm
                            # (the engine would find that out from the note its device side leaves at every close, four windows late; the replay is told)
                            warm=False if big else None)
    g.set_clock(1_000_000_000, 1_700_000_000_000_000_000)
    g.load_weights(weights.make_weights(L))
    for i in range(topo.n_pods):
        g.upsert_pod(int(topo.pod_ips[i]), i)
    for j in range(topo.n_svcs):
        g.upsert_service(int(topo.svc_ips[j]), topo.n_pods + j)
    g.set_label_count(len(labels))
    return g


def churn_leg(a, topo, labels, c, device, dev, Ev, nb, steady_ms):
    """What a window costs when it meets edges the engine has not seen: a fresh engine is warmed on the ring's traces, then
    every window = one of those traces + a small batch of requests on NEW (pod, service) pairs — 0.1 %, 1 % and 4 % of the graph's edges per
    window, drawn at random over all rows, never repeated.  Since round 6 such a window stays warm: the new edges are merged into the
    window's CSR and into the kept set (delta window).  One hipEvent pair per window (timing group 10), median / min over the windows of a
    rate; every window is read back, so sg_stats says which path each one took."""
    import torch
    from alaz_amd import engine, replay, weights
    g = _engine_for(a, topo, labels, c, device, 1, engine, weights)
    P, S, E0 = topo.n_pods, topo.n_svcs, len(topo.edge_src)
    rng = np.random.default_rng(20260930)
    have = (topo.edge_src.astype(np.uint64) << np.uint64(32)) | topo.edge_dst.astype(np.uint64)
    tmpl = np.zeros(1, dtype=replay.EVENT_DTYPE)
    def batch_of_new_edges(n):
        nonlocal have
        src = rng.integers(0, P, size=2 * n + 64).astype(np.uint64); dst = (P + rng.integers(0, S, size=2 * n + 64)).astype(np.uint64)
        key = (src << np.uint64(32)) | dst
        key = np.unique(key[~np.isin(key, have)])
        key = rng.permutation(key)[:n]
        have = np.concatenate([have, key])
        ev = np.repeat(tmpl, 4 * len(key))
        s_ = (key >> np.uint64(32)).astype(np.int64); d_ = (key & np.uint64(0xFFFFFFFF)).astype(np.int64) - P
        ev["saddr"] = np.repeat(topo.pod_ips[s_], 4); ev["daddr"] = np.repeat(topo.svc_ips[d_], 4)
        ev["status"] = 200; ev["protocol"] = 1
        ev["duration_ns"] = rng.integers(1_000_000, 20_000_000, size=len(ev)); ev["write_time_ns"] = 2_000_000_000 + np.arange(len(ev), dtype=np.uint64)
        return torch.from_numpy(ev.view(np.uint8).reshape(-1)).cuda(), len(ev), len(key)
    out = []
    try:
        for i in range(4):                                           # the ring's traces: everything after this is warm unless a window brings something new
            g.ingest_device(dev[i % nb].data_ptr(), Ev, 0); g.window_run(0)
        torch.cuda.synchronize()
        wi = 0
        for rate in (0.001, 0.01, 0.04):
            W = 6
            extra = [batch_of_new_edges(max(1, int(rate * E0))) for _ in range(W)]
            torch.cuda.synchronize()
            before = g.stats()
            g.timing_reset(); g.timing_enable(1 << 10)
            new_seen = []
            for k in range(W):
                g.ingest_device(dev[wi % nb].data_ptr(), Ev, 0); wi += 1
                g.ingest_device(extra[k][0].data_ptr(), extra[k][1], 0)
                g.window_run(0)
                torch.cuda.synchronize()
                g.window_read(); new_seen.append(int(g.stats().last_window_new_edges))
            g.timing_enable(0)
            w = np.sort(g.timing_samples(10, W + 8))
            st = g.stats()
            # the SAME windows once more: their edges are known now — what the window costs without anything new (it has a second,
            # small pass-A launch for the extra batch, which the replay's steady window has not)
            g.timing_reset(); g.timing_enable(1 << 10)
            for k in range(W):
                g.ingest_device(dev[wi % nb].data_ptr(), Ev, 0); wi += 1
                g.ingest_device(extra[k][0].data_ptr(), extra[k][1], 0)
                g.window_run(0)
                torch.cuda.synchronize()
            g.timing_enable(0)
            w2 = np.sort(g.timing_samples(10, W + 8))
            # where the difference goes: per kernel group (event pairs around every group: a few microseconds each, so in passes of their own),
            # two more windows with new edges, then the same two with the edges known
            def groups(batches):
                g.timing_reset(); g.timing_enable(1)
                nonlocal wi
                for b_ in batches:
                    g.ingest_device(dev[wi % nb].data_ptr(), Ev, 0); wi += 1
                    g.ingest_device(b_[0].data_ptr(), b_[1], 0)
                    g.window_run(0)
                torch.cuda.synchronize(); g.timing_enable(0)
                return {name: round(g.timing(k)[0] * g.timing(k)[1] / len(batches), 1) for name, k in (("K1a", 1), ("K1b", 7), ("K2", 2), ("K3-in", 8), ("K3-feat", 3), ("K4", 4), ("K5", 5))}
            more = [batch_of_new_edges(max(1, int(rate * E0))) for _ in range(2)]
            torch.cuda.synchronize()
            grp_new, grp_known = groups(more), groups(more)
            out.append({"new_edges_per_window": extra[0][2], "share_of_graph": rate, "windows": W,
                        "ms_per_window_median": round(float(np.median(w)) / 1e3, 5), "ms_per_window_min": round(float(w[0]) / 1e3, 5),
                        "ms_same_windows_edges_known": round(float(np.median(w2)) / 1e3, 5),
                        "vs_same_windows_edges_known": round(float(np.median(w)) / float(np.median(w2)), 3),
                        "vs_steady_window": round(float(np.median(w)) / 1e3 / steady_ms, 3) if steady_ms else None,
                        "new_edges_merged": new_seen,
                        "us_per_kernel_group": {"with_new_edges": grp_new, "edges_known": grp_known},
                        "paths": {"warm": int(st.windows_warm - before.windows_warm), "of_them_delta": int(st.windows_delta - before.windows_delta),
                                  "cold": int(st.windows_cold - before.windows_cold), "plain": int(st.windows_plain - before.windows_plain)}})
            del extra
    finally:
        g.close()
    return out


def bench_single(a, device):
    from alaz_amd import replay

    cfgno = 3 if a.config == 4 else a.config
    c = replay.CONFIGS[cfgno]
    seed = replay.SEED_BASE + cfgno
    Ev, L = c["events"], c["layers"]
    nb = a.batches or max(2, -(-(320 << 20) // (Ev * 32)))          # ring >= 320 MB > 256 MiB Infinity Cache
    topo = replay.make_topology(c["pods"], c["edges"], seed)
    full_topo = topo
    if a.shard_of > 1:                                               # shard 0 of `shard_of`: its edges, every node (the join tables are replicated)
        from alaz_amd import sharded
        topo = sharded.shard_view(full_topo, 0, a.shard_of)
        Ev = Ev // a.shard_of                                        # its routed share of a window (events are drawn from the shard's own edges)
        nb = a.batches or max(2, -(-(320 << 20) // (Ev * 32)))
    cache = os.environ.get("SG_BENCH_CACHE")                         # tools/gpu.sh: several profiler passes over the same trace on one box
    cpath = os.path.join(cache, f"bench_ev_c{cfgno}_{nb}_s{a.shard_of}.npy") if cache else None
    if cpath and os.path.exists(cpath):
        ev_all = np.load(cpath); labels = list(replay.EXTERNAL_HOSTS)
        labels = labels[: int(ev_all["host_label"].max())]
    else:
        ev_all, labels = replay.make_events(topo, Ev * nb, seed, mixed=(cfgno == 5))
        if cpath:
            np.save(cpath, ev_all)
    cpu = None
    if a.full and not a.no_cpu_baseline and not a.profile_mode:      # before the GPU runtime exists in this process (fork)
        cpu = cpu_baseline(topo, ev_all[:Ev], labels, L, a.cpu_seconds)

    import torch
    from alaz_amd import engine, weights
    torch.cuda.set_device(device)
    g = _engine_for(a, topo, labels, c, device, a.windows, engine, weights)
    s = 0          # NULL stream argument: the engine enqueues every window on its own slot's stream
    dev = [torch.from_numpy(ev_all[i * Ev:(i + 1) * Ev].view(np.uint8).reshape(-1)).cuda() for i in range(nb)]
    torch.cuda.synchronize()

    def step(i):
        g.ingest_device(dev[i % nb].data_ptr(), Ev, s)
        g.window_run(s)

    # Settle: the setup (and with --full the CPU-baseline leg) leaves the GPU idle for seconds and the timed region is only a few
    # milliseconds long — whatever DPM state the chip is in would be what gets timed.  Untimed real windows until
    # the clock is up.
    settle_windows = 0
    if a.settle_ms > 0 and not a.profile_mode:
        ts = time.perf_counter()
        while (time.perf_counter() - ts) * 1e3 < a.settle_ms:
            for _ in range(8):
                step(settle_windows); settle_windows += 1
            torch.cuda.synchronize()
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    clk_before = g.clock_probe(200)                          # (all-CU spin now, pass A of the settle + warm-up windows)
    # dispatch stamps of the K1 launches (pass A + pass B) on their stream, on every third window of the timed steps: the stamps cost a few
    # microseconds per launch (three stamped launches a window moved the timed mean 17 us above the unstamped median), the averages below
    # are still over launches of the timed region.  A plain run takes them too and reads none: the timed steps are the same either way
    stride = 3 if a.steps >= 9 else 1
    g.timing_reset(); g.timing_stride(stride); g.timing_enable((1 << 1) | (1 << 7))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(a.warmup + i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    g.timing_enable(0); g.timing_stride(1)
    if not a.full and not a.profile_mode:
        # a plain run: the headline line, the last timed window's rows if asked, nothing else
        dumped = dump_outputs(a.dump_outputs, g.window_read(), g.outbound_ips()) if a.dump_outputs else None
        geo = g.geometry()
        g.close()
        res = headline(a, cfgno, c, topo, Ev, L, nb, geo, dt)
        if dumped:
            res["dump_outputs"] = dumped
        return res
    clk_after = g.clock_probe(200)                           # (spin right after the timed steps, pass A of exactly the timed steps)
    k1a, k1b = g.timing(1), g.timing(7)
    k1a_s, k1b_s = g.timing_samples(1), g.timing_samples(7)  # every launch of the timed steps, by the dispatch's own stamps
    # an engine that keeps warm-window state launches pass B twice per window (the warm attempt, then the cold merge, which returns at
    # once on a warm window): a window's pass B is the SUM of its launches
    nwin_s = max(1, len(k1a_s))                               # stamped windows (one pass-A launch each: the replay feeds a window in one batch)
    per_w = max(1, round(len(k1b_s) / nwin_s))
    if per_w > 1 and len(k1b_s) == per_w * nwin_s:
        k1b_s = k1b_s.reshape(nwin_s, per_w).sum(axis=1)
        k1b = (float(k1b_s.mean()), nwin_s)
    st_timed = g.stats()
    # --dump-outputs: the rows of the last timed window, read back before anything below ingests again (they stay in place until then)
    dumped = dump_outputs(a.dump_outputs, g.window_read(), g.outbound_ips()) if a.dump_outputs else None
    # SURVEY 8(d) run protocol (median + min): a separate untimed pass — the event pair around every window costs a few microseconds, so it
    # stays out of the region `value` is taken from — of at least 100 windows (or the driver's --steps if that is more), one record each
    # from in front of the window's pass A to behind its score kernel
    per_step = None
    if not a.profile_mode:
        nds = max(100, a.steps) if Ev <= 10_000_000 else max(20, a.steps)
        g.timing_reset(); g.timing_enable(1 << 10)
        for i in range(nds):
            step(i)
        torch.cuda.synchronize()
        g.timing_enable(0)
        w = np.sort(g.timing_samples(10, nds + 8))
        if len(w):
            per_step = {"windows": int(len(w)), "median_ms": round(float(np.median(w)) / 1e3, 5), "min_ms": round(float(w[0]) / 1e3, 5),
                        "p90_ms": round(float(w[int(0.9 * (len(w) - 1))]) / 1e3, 5), "max_ms": round(float(w[-1]) / 1e3, 5),
                        "events_per_s_at_median": Ev / (float(np.median(w)) * 1e-6), "events_per_s_at_min": Ev / (float(w[0]) * 1e-6),
                        "how": "untimed pass behind the timed steps, one hipEvent pair per window on the window's stream (first pass-A launch .. score kernel)"}
    # untimed diagnostic pass: per-group durations of the rest of the window pipeline (hipEvent pairs cost a few us each)
    grp = {}
    nd = min(10, a.steps)
    if not a.profile_mode:
        g.timing_reset(); g.timing_enable(1)
        for i in range(nd):
            step(i)
        torch.cuda.synchronize()
        g.timing_enable(0)
        for name, k in (("K2", 2), ("K3-in", 8), ("K3-feat", 3), ("K4", 4), ("K5", 5)):
            us, n = g.timing(k)
            grp[name] = us * n / nd                                 # per window (a group may have several records per window)

    # the cold path beside the steady state: the same steps with the warm path switched off — every window rebuilt from nothing (what a
    # window costs when its edge set is not among the kept one: first window, new edge, changed node numbering)
    cold = None
    if geo_warm(g) and not a.profile_mode:
        g.set_warm(False)
        for i in range(2):
            step(i)
        g.timing_reset(); g.timing_enable((1 << 1) | (1 << 7))
        torch.cuda.synchronize()
        tc0 = time.perf_counter()
        for i in range(a.steps):
            step(a.warmup + i)
        torch.cuda.synchronize()
        dtc = time.perf_counter() - tc0
        g.timing_enable(0)
        ca, cb = g.timing(1), g.timing(7)
        cold = {"ms_per_step": dtc / a.steps * 1e3, "events_per_s": Ev * a.steps / dtc, "pass_a_us": ca[0], "pass_b_us": cb[0] * cb[1] / max(1, ca[1]),
                "what": "sg_set_warm(0): every window takes the full rebuild (pass B's cold merge with the kept keys carried over, row scan, scatter, row sort of the kept CSR, state capture, then the compaction)"}
        g.set_warm(True)
        for i in range(2):                                   # (back on the warm path for the passes below)
            step(i)
        torch.cuda.synchronize()
    # churn: windows that bring new edges (a fresh engine; this one's kept set stays what the replay made it)
    churn = None
    if geo_warm(g) and not a.profile_mode and a.shard_of == 1 and cfgno != 5 and not a.no_churn:
        try:
            churn = churn_leg(a, topo, labels, c, device, dev, Ev, nb, per_step["median_ms"] if per_step else None)
        except Exception as ex:                              # noqa: BLE001  (a diagnostic leg must never cost the line)
            churn = {"error": repr(ex)[:300]}
    # one untimed window with copy-out: how many edges / nodes a window of this workload has
    g.ingest_device(dev[0].data_ptr(), Ev, s)
    torch.cuda.synchronize()
    rows = g.flush_window()
    st = g.stats()
    E, N = int(st.last_window_edges), int(st.last_window_nodes)
    k1_us = k1a[0] + k1b[0]                                  # K1 = k1a_partition (per batch) + k1b_merge (per window)
    alg = algorithmic_bytes(Ev, E, N, L)
    alg_k1 = alg["K1a"] + alg["K1b"]
    achieved = alg_k1 / (k1_us * 1e-6) / 1e9 if k1_us > 0 else 0.0
    traffic, traffic_src, traffic_match, traffic_cal = pmc_traffic(cfgno)
    kn = g.k1_kernels(); geo = g.geometry()
    copy_gbs = None if a.profile_mode else measured_copy_gbs(torch)
    # which kind of box this line came from (the pool's boxes run the same instruction stream at the same shader clock up to 30 % apart):
    # dependent-load latency through 4 GiB (HBM: far beyond the 256 MiB Infinity Cache, cold) and through 2 MiB walked once before (L2)
    box = None
    if not a.profile_mode:
        try:
            box = {"hbm_latency_ns": round(g.latency_probe(4 << 30, 4096, warm=False), 1), "l2_latency_ns": round(g.latency_probe(2 << 20, 16384, warm=True), 1),
                   "mall_latency_ns": round(g.latency_probe(64 << 20, 16384, warm=True), 1),
                   "hbm_loaded_latency_ns": round(g.latency_probe(4 << 30, 2048, loaded=True), 1),
                   "how": "dependent loads one 128-byte line apart (sg_latency_probe), one lane: 4 GiB cold / 2 MiB warm / 64 MiB warm (Infinity Cache); "
                          "loaded: 65 536 lanes each on a chain of its own through 4 GiB, one timed"}
            pr = torch.cuda.get_device_properties(device)
            box["device"] = {"name": pr.name, "cus": pr.multi_processor_count, "hbm_GiB": round(pr.total_memory / 2**30, 1),
                             "l2_MiB": round(getattr(pr, "L2_cache_size", 0) / 2**20, 1), "gcn_arch": getattr(pr, "gcnArchName", "")}
        except Exception as ex:                              # noqa: BLE001
            box = {"error": repr(ex)[:200]}
    kern_us = {"K1a": k1a[0], "K1b": k1b[0], **grp}
    kernels = [{"name": k, "us_per_window": round(kern_us[k], 2), "algorithmic_bytes": alg[k],
                "GBs": round(alg[k] / (kern_us[k] * 1e-6) / 1e9, 1) if kern_us.get(k, 0) > 0 else None,
                "frac_of_hbm_peak": round(alg[k] / (kern_us[k] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if kern_us.get(k, 0) > 0 else None}
               for k in ("K1a", "K1b", "K2", "K3-in", "K3-feat", "K4", "K5") if k in kern_us]
    b_total = sum(alg.values())
    ms_step = dt / a.steps * 1e3
    res = headline(a, cfgno, c, topo, Ev, L, nb, geo, dt)
    res["config"].update({"edges_per_window": E, "nodes": N, "events_dropped_cap": int(st.events_dropped_cap)})
    res.update({
        "roofline": {"bound": "hbm", "kernel": "K1 resolve_aggregate = " + " + ".join(kn), "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "traffic_calibrated": traffic_cal,   # the same counters divided by their reading for known byte counts in K1's access patterns (profiles/*_pmc_calibration.json)
                     "traffic_source": traffic_src, "traffic_measured_in_run": False, "traffic_build_matches": traffic_match,
                     "measured_copy_GBs": copy_gbs,
                     "frac_of_measured_copy": (achieved / copy_gbs) if copy_gbs else None,
                     "algorithmic_bytes_per_launch": alg_k1, "avg_launch_us": k1_us,
                     "pass_a_us": k1a[0], "pass_b_us": k1b[0], "kernels": list(kn), "launches": k1a[1], "geometry": geo,
                     # (the line's `frac` is the MEAN over the timed launches, as the contract asks; median and minimum of the same launches:)
                     "pass_a_us_median_min": [round(float(np.median(k1a_s)), 2), round(float(k1a_s.min()), 2)] if len(k1a_s) else None,
                     "pass_b_us_median_min": [round(float(np.median(k1b_s)), 2), round(float(k1b_s.min()), 2)] if len(k1b_s) else None,
                     "frac_at_median": (alg_k1 / ((float(np.median(k1a_s)) * (len(k1a_s) / max(1, len(k1b_s))) + float(np.median(k1b_s))) * 1e-6) / 1e9 / HBM_PEAK_GBS) if len(k1a_s) and len(k1b_s) else None},
        "kernels": kernels,
        "window_algorithmic_bytes": b_total, "window_algorithmic_bytes_per_event": b_total / Ev,
        "window_algorithmic_GBs": b_total / (ms_step * 1e-3) / 1e9,
        # shader clock the chip held (MHz = shader cycles per 100 MHz reference tick x 100): under an all-CU integer spin before /
        # after the timed steps, and inside pass A itself, averaged over the launches of the timed steps
        "effective_sclk_mhz": {"spin_before": round(clk_before[0], 1), "spin_after": round(clk_after[0], 1),
                               "pass_a_timed_steps": round(clk_after[1], 1), "pass_a_settle_and_warmup": round(clk_before[1], 1)},
        "settle": {"ms": a.settle_ms if not a.profile_mode else 0.0, "windows": settle_windows},
        "per_step": per_step, "box": box,
        # `value` / ms_per_step are the STEADY STATE of a replay whose windows touch the same edges: every timed window is closed on the warm
        # path (windows_warm_in_check_read says what the window read back at the end was); cold = the same steps with the warm path off
        "warm_windows": {"engine_keeps_state": bool(geo_warm(g)), "cold": cold, "cold_ms_per_step": cold["ms_per_step"] if cold else None,
                         # windows that meet NEW edges (0.1 % / 1 % / 4 % of the graph per window, spread over all rows): merged in, not rebuilt
                         "churn": churn,
                         "windows_read": {"warm": int(st.windows_warm), "cold": int(st.windows_cold)}},
    })
    res["value_basis"] = res.pop("value_basis") + "; per_step holds median / min of single windows"
    if dumped:
        res["dump_outputs"] = dumped
    # diagnostic (never `value`): the same steps with several windows in flight inside one engine — the
    # latency-bound close of window w overlaps the ingest of window w+1; no timing events in this pass
    # (the diagnostic passes below must never cost the line above: an exception in one of them is reported in its object)
    if a.overlap_windows > 1 and not a.profile_mode and cfgno != 5:
        try:
            g2 = _engine_for(a, topo, labels, c, device, a.overlap_windows, engine, weights)
            for i in range(a.warmup):
                g2.ingest_device(dev[i % nb].data_ptr(), Ev, 0); g2.window_run(0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(a.steps):
                g2.ingest_device(dev[(a.warmup + i) % nb].data_ptr(), Ev, 0); g2.window_run(0)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t1
            res["overlapped"] = {"windows_in_flight": a.overlap_windows, "events_per_s": Ev * a.steps / dt2, "ms_per_step": dt2 / a.steps * 1e3}
            g2.close()
        except Exception as ex:                              # noqa: BLE001
            res["overlapped"] = {"error": repr(ex)[:300]}
    # events accepted by sg_ingest from HOST memory until their window's rows are readable on the host
    if not a.no_end_to_end and not a.profile_mode:
        which = os.environ.get("SG_BENCH_E2E", "both")       # (pageable | pinned | both: to look at one of them alone)
        try:
            res["end_to_end"] = end_to_end(g, ev_all, Ev, nb, a.feeders, E) if which != "pinned" else {}
        except Exception as ex:                              # noqa: BLE001
            res["end_to_end"] = {"error": repr(ex)[:300]}
        # the same out of caller memory page-locked with sg_host_register (no staging copy): the copy engine reads hipHostRegister'ed
        # memory at ~47 GB/s against 57 GB/s for the hipHostMalloc'ed staging ring, but the feeders' memcpy is gone
        if which != "pageable":
            try:
                res["end_to_end"]["registered_memory"] = end_to_end(g, ev_all, Ev, nb, a.feeders, E, pinned=True)
            except Exception as ex:                          # noqa: BLE001
                res["end_to_end"]["registered_memory"] = {"error": repr(ex)[:300]}
    e2e = res.get("end_to_end") or {}
    res["value_end_to_end"] = e2e.get("events_per_s")        # host memory -> scored rows on the host (pageable caller memory)
    if cpu is not None:
        res["cpu_baseline"] = cpu
    g.close()
    if cfgno == 5 and a.stream and not a.profile_mode:                 # after the engine above has released its 8 GB of window buffers
        import subprocess
        out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "c5_stream.py")],
                             capture_output=True, text=True, timeout=900)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        res["streaming"] = json.loads(lines[-1]) if lines else {"error": (out.stderr or "no output")[-400:]}
    return res


def end_to_end(g, ev_all, Ev, nb, feeders, E, pinned=False, serial=False):
    """The host feed as the aggregator drives it: `feeders` threads push the events of window after window through sg_ingest (copy into
    the pinned staging ring, H2D on the copy stream, K1a behind it); when a window's Ev events are in, the closer marks the
    boundary (sg_flush_begin: K1b..K5 enqueued), the feeders go on with the next window at once and a fetcher brings the scored
    rows back (sg_flush_end_view) beside that feed, over the other direction of the link.  Every window holds exactly its own
    events; the clock stops when the last window's rows are readable on the host.  pinned: the events sit in memory registered with sg_host_register and go in through
    sg_ingest_pinned.  serial: every feeder stops at the boundary and sg_flush_window_view does the close in one call (round 2)."""
    import torch
    chunk = g.max_batch
    nwin = 4 if Ev >= 5_000_000 else 10
    retries = [0] * feeders
    if pinned:
        g.host_register(ev_all)
    nchunks_w = -(-Ev // chunk)                              # batches per window
    total_chunks = nchunks_w * nwin
    def chunk_of(j):                                         # batch j of the stream: windows cycle through the nb host-resident traces
        w, c = divmod(j, nchunks_w)
        base = (w % nb) * Ev
        return ev_all[base + c * chunk: base + min(Ev, (c + 1) * chunk)]
    rows_seen, ev_seen = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if serial:
        for wdx in range(nwin):
            def feed(k, wdx=wdx):
                for c in range(k, nchunks_w, feeders): retries[k] += g.ingest_bulk(chunk_of(wdx * nchunks_w + c), pinned=pinned)
            ths = [threading.Thread(target=feed, args=(k,)) for k in range(feeders)]
            for t in ths: t.start()
            for t in ths: t.join()
            rows_seen.append(len(g.flush_window_view()))
    else:
        closed = [0]                                         # windows whose boundary has been marked (sg_flush_begin returned)
        done_w = [[0] * feeders for _ in range(nwin)]        # events handed over, per window and feeder
        errs = []
        def feed(k):                                         # sg_ingest_bulk waits for a staging slot instead of dropping (production: drop + count)
            try:
                for j in range(k, total_chunks, feeders):
                    wj = j // nchunks_w
                    while closed[0] < wj and not errs: time.sleep(0.00005)   # a window's events go in after the previous boundary, never before
                    if errs: return
                    p = chunk_of(j)
                    retries[k] += g.ingest_bulk(p, pinned=pinned)
                    done_w[wj][k] += len(p)
            except Exception as ex:                          # noqa: BLE001  (reported by the closer: no thread may wait for a dead one)
                errs.append(ex)
        ths = [threading.Thread(target=feed, args=(k,)) for k in range(feeders)]
        for t in ths: t.start()
        fetch = None
        def fetch_rows():                                    # rows readable in the engine's page-locked host buffer
            try: rows_seen.append(len(g.flush_end_view()))
            except Exception as ex: errs.append(ex)          # noqa: BLE001
        try:
            for wdx in range(nwin):
                while sum(done_w[wdx]) < Ev and not errs: time.sleep(0.00005)
                if fetch: fetch.join()
                if errs: break
                g.flush_begin()                              # the boundary; the feeders go on with the next window at once,
                closed[0] = wdx + 1
                fetch = threading.Thread(target=fetch_rows); fetch.start()   # its rows come back over the other direction of the link meanwhile
        except Exception as ex:                              # noqa: BLE001
            errs.append(ex)
        for t in ths: t.join()
        if fetch: fetch.join()
        if errs:
            if pinned: g.host_unregister(ev_all)
            raise errs[0]
    dt = time.perf_counter() - t0
    rows_n = int(sum(rows_seen) / max(1, len(rows_seen)))
    dropped_ring = int(g.stats().events_dropped_ring)       # (sg_ingest_bulk waits instead of dropping: stays 0)
    # what the link itself does on this box: pinned 256 MiB copies, best of 3 (the bound the figure above is held against)
    hp = torch.empty(256 << 20, dtype=torch.uint8).pin_memory(); dv = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    h2d = d2h = 0.0
    for _ in range(3):
        torch.cuda.synchronize(); t1 = time.perf_counter(); dv.copy_(hp, non_blocking=True); torch.cuda.synchronize(); h2d = max(h2d, (256 << 20) / (time.perf_counter() - t1) / 1e9)
        torch.cuda.synchronize(); t1 = time.perf_counter(); hp.copy_(dv, non_blocking=True); torch.cuda.synchronize(); d2h = max(d2h, (256 << 20) / (time.perf_counter() - t1) / 1e9)
    link_ms = (32.0 * Ev / h2d + 64.0 * E / d2h) / 1e6       # the bound of rounds 1-2: both transfers of a window, one after the other
    duplex_ms = max(32.0 * Ev / h2d, 64.0 * E / d2h) / 1e6   # if the two directions of the link did not disturb each other at all
    if pinned:
        g.host_unregister(ev_all)
    return {"entry_point": "sg_ingest_pinned (events in registered page-locked memory, no staging copy)" if pinned else "sg_ingest (pageable caller memory, copied into the pinned staging ring)",
            "events_per_s": Ev * nwin / dt, "ms_per_window": dt / nwin * 1e3, "windows": nwin, "feeders": feeders,
            "pcie_measured_GBs": {"h2d": round(h2d, 1), "d2h": round(d2h, 1)}, "pcie_bound_ms_per_window": round(link_ms, 3),
            "frac_of_pcie_bound": round(link_ms / (dt / nwin * 1e3), 3),
            "pcie_duplex_ms_per_window": round(duplex_ms, 3), "frac_of_duplex_bound": round(duplex_ms / (dt / nwin * 1e3), 3),
            "includes": ([] if pinned else ["memcpy into pinned staging ring"]) + ["h2d (own stream, overlapping K1a of the previous batch)", f"K1a per staging batch ({chunk} events, copied and sent in 4 MiB pieces)", "K1b..K5", "d2h of the scored rows into page-locked host memory (sg_flush_begin / sg_flush_end_view: beside the next window's feed)", "window reset"],
            "rows_per_window": rows_n, "rows_by_window": rows_seen, "ring_full_retries": int(sum(retries)), "events_dropped_ring": dropped_ring,
            "bound": f"PCIe: 32 B/event host->device + 64 B/edge device->host ({(32.0 * Ev + 64.0 * E) / 1e6:.0f} MB per window) at the measured one-direction rates; duplex = the larger of the two alone (measured: the H2D slows down while the D2H runs)"}


if __name__ == "__main__":
    sys.exit(main() or 0)
