"""ctypes front end of libservicegraph.so (the C ABI of include/servicegraph.h).

This module is plumbing: it owns no algorithm.  Every result it returns was produced by the HIP
kernels behind the C ABI.  If the library is missing, or no gfx950 device is usable, it raises —
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np

from .replay import EDGE_OUT_DTYPE, EVENT_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SG_LIB_PATH") or os.path.join(_HERE, "lib", "libservicegraph.so")   # SG_LIB_PATH: A/B runs of two builds on one box
# the development build (-DSG_DEV_KNOBS, alaz_amd/build.py): the only one that reads SG_* tuning knobs from the environment and has the
# SG_ABLATE bits / phase stamps compiled in.  ServiceGraph(dev_knobs=True) — tools/, the A/B tests of alternative kernel paths — loads it.
LIB_DEV_PATH = os.path.join(_HERE, "lib", "libservicegraph_dev.so")
#: the knobs the development build reads (csrc/sg_plan.hpp kKnobs); ServiceGraph(dev_knobs=None) picks that build when one of them is set
DEV_KNOBS = ("SG_ABLATE", "SG_NP", "SG_HT", "SG_CT", "SG_NWG", "SG_NSUB", "SG_SPLIT", "SG_WARM", "SG_K1A", "SG_K1_NARROW", "SG_K1_LEGACY", "SG_K1B_U",
             "SG_K1B_THREADS", "SG_K1B_PACK", "SG_K1B_NO_ORDER", "SG_L2_GLOBAL", "SG_L2_U32", "SG_DH_G", "SG_K3_SLICES", "SG_K3_NO_FUSE", "SG_K4_FUSED", "SG_K5_GRID", "SG_K6_ONE_WG", "SG_DENSE_VALU",
             "SG_COPY_STREAMS", "SG_STAGE_SLOTS", "SG_ARENA", "SG_NO_FOLD", "SG_K1A_PAIR", "SG_K5_FORM", "SG_K5_EFEAT", "SG_K3_IN_FORM", "SG_K3_FEAT_LANES")

SG_OK, SG_EINVAL, SG_ENOMEM, SG_ENODEV, SG_ENOSPC, SG_EAGAIN, SG_ESTATE = 0, -22, -12, -19, -28, -11, -71
SELECT_MAX_K = 16384      # SG_SELECT_MAX_K: the largest k of a top-k selection
F_IN, F_HID, F_EDGE = 32, 64, 8
STAT_SUM_WORDS, STAT_MAX_WORDS = 12, 2
REF_KNOWN, REF_LABEL, REF_OBIP = 0, 1, 2

#: sg_edge_trend (16 bytes) and sg_trend_entry (56 bytes) of include/servicegraph.h
TREND_DTYPE = np.dtype([("lat_dev", "<f4"), ("err_dev", "<f4"), ("base_mean_us", "<f4"), ("windows_seen", "<u4")])
TREND_ENTRY_DTYPE = np.dtype([("from_key", "<u8"), ("to_key", "<u8"), ("lat_mean", "<f8"), ("lat_dev", "<f8"), ("err_mean", "<f8"),
                              ("err_dev", "<f8"), ("n", "<u4"), ("last", "<u4")])
#: sg_node_out (136 bytes) of include/servicegraph.h: one node of a window's rollup (K9)
NODE_DTYPE = np.dtype([(f"{side}_{f}", "<u8") for f in ("count", "err", "sum_ns", "sumsq_us", "max_ns", "score_q32") for side in ("out", "in")]
                      + [(f, "<u4") for f in ("ref", "out_edges", "in_edges", "out_alive", "in_alive", "out_worst_row", "in_worst_row")]
                      + [(f, "<f4") for f in ("out_score_max", "in_score_max", "score")])
#: sg_node_trend (32 bytes) of include/servicegraph.h: one node row's two sides against the node baseline (K10)
NODE_TREND_DTYPE = np.dtype([(f, "<f4") for f in ("in_lat_dev", "in_err_dev", "out_lat_dev", "out_err_dev", "in_base_mean_us", "out_base_mean_us")]
                            + [("in_seen", "<u4"), ("out_seen", "<u4")])
#: sg_node_rank (16 bytes) of include/servicegraph.h: one node row's culprit rank (K11); share = rank * 2^-56
RANK_DTYPE = np.dtype([("rank", "<u8"), ("ref", "<u4"), ("share", "<f4")])
#: SG_RANK_SEED_*: where the walk restarts
RANK_SEED = dict(score=0, uniform=1)
#: sg_rank_params defaults (a 0 in the struct means the same: iters 20, damping_q8 218)
RANK_DEFAULTS = dict(iters=0, damping_q8=0, seed="score", seed_min_score=0.0)
#: sg_incident_out (72 bytes) of include/servicegraph.h: one incident of a window (K12), a connected component of its red rows
INCIDENT_DTYPE = np.dtype([(f, "<u8") for f in ("count", "err", "sum_ns", "score_q32", "rank_sum")]
                          + [(f, "<u4") for f in ("first_node", "nodes", "edges", "worst_row", "top_node", "culprit_node")]
                          + [("value_max", "<f4"), ("reserved", "<u4")])
#: SG_NO_INCIDENT: a node row in no incident; culprit_node with the ranking off
NO_INCIDENT = 0xFFFFFFFF
#: sg_incident_params defaults
INCIDENT_DEFAULTS = dict(by="score", min_value=0.0)
#: sg_incident_track (32 bytes) of include/servicegraph.h: the track of one incident of a window (K13)
TRACK_DTYPE = np.dtype([(f, "<u4") for f in ("track", "parent", "first_window", "windows", "kept_nodes", "moved_nodes", "joined_nodes", "flags")])
#: sg_track_entry (40 bytes) of include/servicegraph.h: one entry of the track table, and of a window's ended list
TRACK_ENTRY_DTYPE = np.dtype([(f, "<u4") for f in ("track", "parent", "first_window", "last_window", "windows", "peak_nodes")]
                             + [("count", "<u8"), ("err", "<u8")])
#: SG_NO_TRACK: no track (the parent of a track that continues none), and sg_incident_track.flags' SG_TRACK_* bits
NO_TRACK = 0xFFFFFFFF
TRACK_NEW, TRACK_SPLIT, TRACK_MERGED = 1, 2, 4
#: sg_track_params defaults (max_tracks 0 = never cut)
TRACK_DEFAULTS = dict(quiet_windows=2, max_tracks=0)
#: sg_group_edge (80 bytes) of include/servicegraph.h: one edge of a window's service map contracted to workloads (K14)
GROUP_EDGE_DTYPE = np.dtype([(f, "<u8") for f in ("count", "err_count", "sum_ns", "sumsq_us", "max_ns", "score_q32")]
                            + [(f, "<u4") for f in ("from_ref", "to_ref", "edges", "from_nodes", "first", "alive", "worst_row")]
                            + [("score_max", "<f4")])
#: SG_NO_GROUP: a node in no group; SG_REF_GROUP: the ref type of a group in sg_group_edge.from_ref / to_ref
NO_GROUP = 0xFFFFFFFF
REF_GROUP = 3
#: sg_group_params defaults (max_groups 0 = max_known_nodes)
GROUP_DEFAULTS = dict(max_groups=0)
#: sg_edge_vanished (64 bytes) of include/servicegraph.h: one baseline entry that went silent (K8's vanished list)
VANISHED_DTYPE = np.dtype([("from_key", "<u8"), ("to_key", "<u8"), ("lat_mean", "<f8"), ("lat_dev", "<f8"), ("err_mean", "<f8"),
                           ("err_dev", "<f8"), ("n", "<u4"), ("last", "<u4"), ("row", "<u4"), ("reserved", "<u4")])
#: sg_vanished_params defaults (a 0 in the struct means the same: silent_windows 1, min_seen = the trend's warmup, max_rows =
#: min(65536, max_entries))
VANISHED_DEFAULTS = dict(silent_windows=0, min_seen=0, max_rows=0)
#: SG_SEL_*: the key of a selection
SEL_BY = dict(score=0, lat_dev=1, err_dev=2, new=3)
#: SG_NSEL_*: the key of a node selection
NSEL_BY = dict(score=0, in_lat_dev=1, in_err_dev=2, out_lat_dev=3, out_err_dev=4, new=5)
#: sg_trend_params defaults (a 0 in the struct means the same)
TREND_DEFAULTS = dict(shift=4, warmup=4, ttl=64, max_entries=0, lat_floor_ns=1000, err_floor=10486)
#: SG_Q_*: the spaces of the latency percentiles (K20), and SG_Q_MAX, the quantiles per entity and side at most
Q_SPACES = dict(nodes=1, groups=2, group_nodes=4)
Q_MAX = 8
#: SG_T_*: the spaces of the traffic baselines (K23); SG_TSEL_*: the key of a selection by a traffic row — a direction, on the
#: node-shaped spaces ORed with a side; sg_traffic_params defaults (a 0 in the struct means the same: rate_floor 8 requests,
#: load_floor_ns 1 000 000)
T_SPACES = dict(edges=1, nodes=2, groups=4, group_nodes=8)
TSEL_BY = dict(surge=0, drop=1, load_up=2, load_down=3)
TSEL_SIDE = {"in": 4, "out": 8}
TRAFFIC_DEFAULTS = dict(shift=4, warmup=4, ttl=64, max_entries=0, load_floor_ns=1000000, rate_floor=8)
#: SG_SLO_*: an SLO row (K24) is SLO_WORDS u64 words — SLO_SIDE_FIELDS for the in side (words 0 .. 7), again for the out side
#: (8 .. 15), flags | objective << 32, then the windows the short | long << 32 span covers; a state entry is SLO_ENTRY_WORDS words
#: (the key, the twelve sums, the objective word).  SLOSEL_*: the key of a selection by a burn rate, a kind ORed with a side.
#: SLO_DEFAULTS: 99 % below 2^27 ns (134 ms), 99.9 % without error, over 2 and 12 windows, the 14.4 x burn of a page
SLO_WORDS = 18
SLO_ENTRY_WORDS = 14
SLO_MAX_WINDOWS = 64
SLO_SIDE_FIELDS = ("total_short", "err_short", "slow_short", "total_long", "err_long", "slow_long", "burn_err", "burn_slow")
SLO_UNTRACKED, SLO_ERR_BURNING_IN, SLO_SLOW_BURNING_IN, SLO_ERR_BURNING_OUT, SLO_SLOW_BURNING_OUT = 1, 2, 4, 8, 16
SLOSEL_BY = dict(err=0, slow=1)
SLOSEL_SIDE = {"in": 2, "out": 4}
SLO_DEFAULTS = dict(latency_bin=10, latency_target_ppm=990000, error_target_ppm=999000, short_windows=2, long_windows=12, min_burn_q10=14746,
                    min_requests=100)
#: SG_IMPACT_*: an impact row of the workload impact (K22) is IMPACT_WORDS u64 words, named by IMPACT_FIELDS in word order; the
#: parameters' limits; SG_NO_HOPS: a workload row no covered incident reaches within max_hops
IMPACT_WORDS = 8
IMPACT_MAX_INCIDENTS = 1024
IMPACT_MAX_HOPS = 64
NO_HOPS = 0xFFFFFFFF
IMPACT_FIELDS = ("exposed", "direct", "far", "entries", "entry_count", "entry_err", "into_count", "into_err")
IMPACT_EXPOSED, IMPACT_DIRECT, IMPACT_FAR, IMPACT_ENTRIES, IMPACT_ENTRY_COUNT, IMPACT_ENTRY_ERR, IMPACT_INTO_COUNT, IMPACT_INTO_ERR = range(8)


class SgConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("device", C.c_int32), ("max_known_nodes", C.c_uint32),
                ("max_labels", C.c_uint32), ("max_outbound_ips", C.c_uint32), ("max_ips", C.c_uint32),
                ("max_edges", C.c_uint64), ("max_batch", C.c_uint32), ("layers", C.c_uint32),
                ("rank", C.c_uint32), ("world", C.c_uint32), ("k1_variant", C.c_uint32),
                ("max_window_events", C.c_uint64), ("windows_in_flight", C.c_uint32), ("max_alive", C.c_uint32), ("flags", C.c_uint32)]


CFG_EDGE_HISTOGRAM = 1
CFG_NO_WARM = 2
CFG_WARM = 4
ABI_VERSION = 6


def make_config(*, max_known_nodes: int, max_edges: int, layers: int = 1, max_labels: int = 256, max_outbound_ips: int = 64,
                max_ips: int = 0, max_batch: int = 1 << 16, device: int = 0, rank: int = 0, world: int = 1, k1_variant: int = 0,
                max_window_events: int = 0, windows_in_flight: int = 1, max_alive: int = 0, flags: int = 0) -> "SgConfig":
    """sg_config by field name (struct_size and abi_version filled in)."""
    return SgConfig(C.sizeof(SgConfig), ABI_VERSION, device, max_known_nodes, max_labels, max_outbound_ips, max_ips or max_known_nodes,
                    max_edges, max_batch, layers, rank, world, k1_variant, max_window_events, windows_in_flight, max_alive, flags)


class SgGeometry(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("k1_variant", "k1_narrow", "partitions", "table_slots", "pass_a_workgroups", "cache_slots",
                                          "join_l2_in_lds", "tile_records", "endpoint_bits", "piece_bytes", "pass_b_split", "pass_a_teams", "warm_windows")]


class SgStats(C.Structure):
    _fields_ = [("events_in", C.c_uint64), ("events_dropped_src", C.c_uint64), ("events_dropped_ring", C.c_uint64),
                ("events_dropped_cap", C.c_uint64), ("windows", C.c_uint64), ("last_window_events", C.c_uint64),
                ("last_window_edges", C.c_uint64), ("last_window_nodes", C.c_uint64),
                ("last_window_tmin_ms", C.c_int64), ("last_window_tmax_ms", C.c_int64), ("h2d_bytes", C.c_uint64),
                ("events_misrouted", C.c_uint64), ("halo_overflow", C.c_uint64),
                ("alive_in", C.c_uint64), ("alive_dropped", C.c_uint64),
                ("join_word_updates", C.c_uint64), ("join_full_uploads", C.c_uint64), ("ingest_waits", C.c_uint64),
                ("windows_warm", C.c_uint64), ("windows_cold", C.c_uint64),
                ("windows_delta", C.c_uint64), ("windows_plain", C.c_uint64), ("last_window_new_edges", C.c_uint64)]


class SgTrendParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("shift", C.c_uint32), ("warmup", C.c_uint32), ("ttl", C.c_uint32),
                ("max_entries", C.c_uint64), ("lat_floor_ns", C.c_uint64), ("err_floor", C.c_uint32), ("reserved", C.c_uint32)]


class TrafficParams(C.Structure):
    """sg_traffic_params (K23); tests/test_traffic_host.py holds its layout to the header with the compiler"""
    _fields_ = [("struct_size", C.c_uint32), ("shift", C.c_uint32), ("warmup", C.c_uint32), ("ttl", C.c_uint32),
                ("max_entries", C.c_uint64), ("load_floor_ns", C.c_uint64), ("rate_floor", C.c_uint32), ("reserved", C.c_uint32)]


class SloParams(C.Structure):
    """sg_slo_params (K24); tests/test_slo_host.py holds its layout to the header with the compiler"""
    _fields_ = [("struct_size", C.c_uint32), ("latency_bin", C.c_uint32), ("latency_target_ppm", C.c_uint32), ("error_target_ppm", C.c_uint32),
                ("short_windows", C.c_uint32), ("long_windows", C.c_uint32), ("min_burn_q10", C.c_uint32), ("reserved", C.c_uint32),
                ("min_requests", C.c_uint64)]


class SloStats(C.Structure):
    """sg_slo_stats (K24)"""
    _fields_ = [(n, C.c_uint64) for n in ("windows", "keys_active", "sides_burning", "keys")]


def slo_budget_code(budget_ppm: int) -> int:
    """SG_SLO_BUDGET_CODE of a budget in ppm: exp << 10 | mant with budget = mant * 10^exp, mant 1 .. 1000 — the smallest exp that
    holds it; ValueError for a budget that has more than three significant digits or lies outside 1 .. 999 999"""
    for exp in range(4):
        mant, rest = divmod(budget_ppm, 10 ** exp)
        if rest == 0 and 1 <= mant <= 1000 and budget_ppm <= 999999:
            return exp << 10 | mant
    raise ValueError(f"a budget of {budget_ppm} ppm is no mant * 10^exp with mant 1 .. 1000, exp 0 .. 3")


def slo_objective(latency_bin: int, latency_target_ppm: int, error_target_ppm: int) -> int:
    """SG_SLO_OBJECTIVE: the objective word of sg_slo_assign from a bin (0 .. 14) and two targets in ppm"""
    if not 0 <= latency_bin <= 14:
        raise ValueError("latency_bin is 0 .. 14")
    return latency_bin << 28 | slo_budget_code(1000000 - latency_target_ppm) << 12 | slo_budget_code(1000000 - error_target_ppm)


#: SG_REPL_* / SG_RSEL_* (K25): a pod row is REPLICA_WORDS u32 words — the workload row index (0xFFFFFFFF: no member), the flags, then
#: REPLICA_SIDE_FIELDS for the in side (words 2 .. 6) and again for the out side (7 .. 11); a workload row is REPLICA_GROUP_WORDS
#: words, REPLICA_GROUP_FIELDS a side.  A side's flags are the in side's << 4 * side.  REPLICA_DEFAULTS: every 0 is the stage's own default
REPLICA_WORDS = 12
REPLICA_GROUP_WORDS = 8
REPLICA_SIDE_FIELDS = ("err_excess_q20", "lat_ratio_q10", "share_q10", "tail_bins", "replicas")
REPLICA_GROUP_FIELDS = ("replicas", "judged", "outliers", "first_outlier")
REPL_MEMBER, REPL_JUDGED_IN, REPL_ERR_IN, REPL_LAT_IN, REPL_TAIL_IN = 1, 2, 4, 8, 16
REPL_JUDGED_OUT, REPL_ERR_OUT, REPL_LAT_OUT, REPL_TAIL_OUT = 32, 64, 128, 256
RSEL_BY = dict(err=0, lat=1, tail=2, share=3)
RSEL_SIDE = {"in": 4, "out": 8}
REPLICA_DEFAULTS = dict(min_replicas=0, min_requests=0, min_err_excess_q20=0, min_lat_ratio_q10=0, tail_permille=0, min_tail_bins=0)


class ReplicaParams(C.Structure):
    """sg_replica_params (K25); tests/test_replicas_host.py holds its layout to the header with the compiler"""
    _fields_ = [("struct_size", C.c_uint32), ("min_replicas", C.c_uint32), ("min_requests", C.c_uint64), ("min_err_excess_q20", C.c_uint32),
                ("min_lat_ratio_q10", C.c_uint32), ("tail_permille", C.c_uint32), ("min_tail_bins", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class SgVanishedParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("silent_windows", C.c_uint32), ("min_seen", C.c_uint32), ("max_rows", C.c_uint32)]


class SgRankParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iters", C.c_uint32), ("damping_q8", C.c_uint32), ("seed", C.c_uint32),
                ("seed_min_score", C.c_float), ("reserved", C.c_uint32)]


class SgIncidentParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("by", C.c_uint32), ("min_value", C.c_float), ("reserved", C.c_uint32)]


class SgGroupParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_groups", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class SgTrackParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("quiet_windows", C.c_uint32), ("max_tracks", C.c_uint32), ("reserved", C.c_uint32)]


class SgTrackStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("windows", "live", "opened", "dropped_cap")]


class SgTrendStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("windows", "entries", "inserted", "expired", "dropped")]


def _signatures() -> dict:
    """name -> (result type, argument types) of every function include/servicegraph.h declares"""
    I, H, P, PP = C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)
    u32, u64, sz, f32 = C.c_uint32, C.c_uint64, C.c_size_t, C.c_float
    Psz, Pu64, Pf64 = C.POINTER(sz), C.POINTER(u64), C.POINTER(C.c_double)
    return {
        "sg_abi_version": (u32, []), "sg_weights_count": (sz, [u32]), "sg_hash32": (u32, [u32]),
        "sg_last_error": (C.c_char_p, [H]),
        "sg_create": (I, [C.POINTER(SgConfig), PP]), "sg_destroy": (I, [H]),
        "sg_upsert_pod": (I, [H, u32, u32]), "sg_delete_pod": (I, [H, u32]),
        "sg_upsert_service": (I, [H, u32, u32]), "sg_delete_service": (I, [H, u32]),
        "sg_set_clock": (I, [H, u64, u64]), "sg_set_label_count": (I, [H, u32]),
        "sg_load_weights": (I, [H, P, sz]),
        "sg_ingest": (I, [H, P, sz]), "sg_ingest_device": (I, [H, P, sz, P]),
        "sg_flush_window": (I, [H, u64, P, sz, Psz]),
        "sg_flush_window_view": (I, [H, u64, PP, Psz]),
        "sg_flush_begin": (I, [H, u64]),
        "sg_flush_end": (I, [H, P, sz, Psz]),
        "sg_flush_end_view": (I, [H, PP, Psz]),
        "sg_window_run": (I, [H, P]), "sg_window_rows_buffer": (I, [H, PP]),
        "sg_window_close": (I, [H, P]),
        "sg_window_obip_list": (I, [H, P, u32, P, P]),
        "sg_bind_buffers": (I, [H, P, P, PP, u32]),
        "sg_window_close_sharded": (I, [H, P, P, P]),
        "sg_window_features": (I, [H, P]), "sg_window_layer": (I, [H, u32, P]),
        "sg_window_score": (I, [H, P]), "sg_window_score_reset": (I, [H, P]), "sg_window_read": (I, [H, P, sz, Psz]),
        "sg_window_reset": (I, [H, P]),
        "sg_window_buffers": (I, [H, PP, PP, PP, Psz]),
        "sg_window_feat_buffer": (I, [H, u32, PP, Psz]),
        "sg_halo_build": (I, [H, P, u32, P, P]), "sg_halo_pack": (I, [H, u32, P, u32, P, P]),
        "sg_halo_unpack": (I, [H, u32, P, u32, P, P]),
        "sg_window_close_gathered": (I, [H, P, u32, u32, P]),
        "sg_halo_build_padded": (I, [H, P, u32, P]), "sg_halo_pack_padded": (I, [H, u32, P, u32, P, P]),
        "sg_halo_unpack_padded": (I, [H, u32, P, u32, P, P]),
        "sg_window_outbound_ips": (I, [H, P, sz, Psz]),
        "sg_stats_get": (I, [H, C.POINTER(SgStats)]),
        "sg_timing_enable": (I, [H, I]), "sg_timing_reset": (I, [H]),
        "sg_timing_get": (I, [H, I, Pf64, Pu64]),
        "sg_set_warm": (I, [H, I]), "sg_timing_stride": (I, [H, u32]),
        "sg_timing_samples": (I, [H, I, Pf64, sz, Psz]),
        "sg_latency_probe": (I, [H, u64, u32, I, Pf64]),
        "sg_debug_stamps": (I, [H, P, sz]),
        "sg_clock_probe": (I, [H, u32, Pf64, Pf64]),
        "sg_comm_probe": (I, []), "sg_window_halo_counts": (I, [H, P, sz]),
        "sg_route": (I, [H, P, sz, u32, P]),
        "sg_window_hist": (I, [H, P, sz, Psz]),
        "sg_geometry_get": (I, [H, C.POINTER(SgGeometry)]),
        "sg_prepare_fold_get": (I, [H, C.POINTER(u32)]),
        "sg_pass_a_pair_get": (I, [H, C.POINTER(u32)]),
        "sg_k5_form_get": (I, [H, C.POINTER(u32)]),
        "sg_k5_efeat_get": (I, [H, C.POINTER(u32)]),
        "sg_k3_forms_get": (I, [H, C.POINTER(u32), C.POINTER(u32)]),
        "sg_comm_unique_id": (I, [P, sz]), "sg_comm_create": (I, [P, sz, I, I, I, PP]),
        "sg_comm_destroy": (I, [P]), "sg_window_run_sharded": (I, [H, P, P]),
        "sg_host_register": (I, [H, P, sz]), "sg_host_unregister": (I, [H, P]), "sg_ingest_pinned": (I, [H, P, sz]),
        "sg_ingest_bulk": (I, [H, P, sz, I, Pu64]),
        "sg_flush_window_top": (I, [H, u64, u32, f32, P, P, sz, Psz, Psz]),
        "sg_flush_end_top": (I, [H, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_select": (I, [H, u32, f32, P, P, sz, P, P]),
        "sg_set_trend": (I, [H, P]), "sg_window_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_trend_buffer": (I, [H, PP]), "sg_trend_entries": (I, [H, P, sz, Psz]),
        "sg_trend_stats_get": (I, [H, P]),
        "sg_set_nodes": (I, [H, I]), "sg_window_nodes": (I, [H, P, sz, Psz]),
        "sg_window_nodes_buffer": (I, [H, PP, PP]),
        "sg_set_vanished": (I, [H, P]), "sg_window_vanished": (I, [H, P, sz, Psz]),
        "sg_window_vanished_buffer": (I, [H, PP, PP]),
        "sg_flush_window_top_by": (I, [H, u64, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_flush_end_top_by": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_select_by": (I, [H, u32, u32, f32, P, P, sz, P, P]),
        "sg_set_node_trend": (I, [H, P]), "sg_window_node_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_node_trend_buffer": (I, [H, PP]), "sg_node_trend_entries": (I, [H, P, sz, Psz]),
        "sg_node_trend_stats_get": (I, [H, P]),
        "sg_window_nodes_top": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_nodes_select": (I, [H, u32, u32, f32, P, P, sz, P, P]),
        "sg_set_rank": (I, [H, P]), "sg_window_rank": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_rank_buffer": (I, [H, PP]),
        "sg_window_rank_top": (I, [H, u32, f32, P, P, P, sz, Psz, Psz]),
        "sg_window_rank_select": (I, [H, u32, f32, P, P, sz, P, P]),
        "sg_set_incidents": (I, [H, P]), "sg_window_incidents": (I, [H, P, sz, Psz]),
        "sg_window_node_incident": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_incidents_buffer": (I, [H, PP, PP, PP]),
        "sg_set_tracks": (I, [H, P]), "sg_window_incident_tracks": (I, [H, P, sz, Psz]),
        "sg_window_tracks_ended": (I, [H, P, sz, Psz]),
        "sg_window_tracks_buffer": (I, [H, PP, PP, PP]),
        "sg_track_entries": (I, [H, P, sz, Psz]), "sg_track_stats_get": (I, [H, P]),
        "sg_set_groups": (I, [H, P]), "sg_group_assign": (I, [H, P, P, sz]),
        "sg_window_groups": (I, [H, P, sz, Psz]), "sg_window_row_group": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_perm": (I, [H, P, sz, Psz]),
        "sg_window_groups_buffer": (I, [H] + [PP] * 4),
        "sg_set_group_trend": (I, [H, P]), "sg_window_group_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_trend_buffer": (I, [H, PP]), "sg_group_trend_entries": (I, [H, P, sz, Psz]),
        "sg_group_trend_stats_get": (I, [H, P]),
        "sg_set_group_vanished": (I, [H, P]), "sg_window_group_vanished": (I, [H, P, sz, Psz]),
        "sg_window_group_vanished_buffer": (I, [H, PP, PP]),
        "sg_window_groups_top": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_groups_select": (I, [H, u32, u32, f32, P, P, sz, P, P]),
        "sg_set_group_nodes": (I, [H, I]), "sg_window_group_nodes": (I, [H, P, sz, Psz]),
        "sg_window_group_nodes_buffer": (I, [H, PP, PP]),
        "sg_set_group_node_trend": (I, [H, P]), "sg_window_group_node_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_node_trend_buffer": (I, [H, PP]), "sg_group_node_trend_entries": (I, [H, P, sz, Psz]),
        "sg_group_node_trend_stats_get": (I, [H, P]),
        "sg_window_group_nodes_top": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_group_nodes_select": (I, [H, u32, u32, f32, P, P, sz, P, P]),
        "sg_set_group_rank": (I, [H, P]), "sg_window_group_rank": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_rank_buffer": (I, [H, PP]),
        "sg_window_group_rank_top": (I, [H, u32, f32, P, P, P, sz, Psz, Psz]),
        "sg_window_group_rank_select": (I, [H, u32, f32, P, P, sz, P, P]),
        "sg_set_group_incidents": (I, [H, P]), "sg_window_group_incidents": (I, [H, P, sz, Psz]),
        "sg_window_group_node_incident": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_incidents_buffer": (I, [H, PP, PP, PP]),
        "sg_set_group_tracks": (I, [H, P]), "sg_window_group_incident_tracks": (I, [H, P, sz, Psz]),
        "sg_window_group_tracks_ended": (I, [H, P, sz, Psz]),
        "sg_window_group_tracks_buffer": (I, [H, PP, PP, PP]),
        "sg_group_track_entries": (I, [H, P, sz, Psz]), "sg_group_track_stats_get": (I, [H, P]),
        "sg_set_group_impact": (I, [H, u32, u32]), "sg_window_group_impact": (I, [H, P, sz, Psz]),
        "sg_window_group_node_hops": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_impact_mask": (I, [H, P, sz, Psz, C.POINTER(u32)]),
        "sg_window_group_impact_buffer": (I, [H, PP, PP, PP, PP]),
        "sg_set_quantiles": (I, [H, u32, P, sz]),
        "sg_window_node_hist": (I, [H, P, sz, P, sz, Psz]), "sg_window_node_quantiles": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_hist": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_quantiles": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_node_hist": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_node_quantiles": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_quantiles_buffer": (I, [H, u32, PP, PP]),
        "sg_set_quantile_trend": (I, [H, u32, u32, P]),
        "sg_window_node_quantile_trend": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_quantile_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_node_quantile_trend": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_quantile_trend_buffer": (I, [H, u32, PP]),
        "sg_quantile_trend_entries": (I, [H, u32, P, sz, Psz]), "sg_quantile_trend_stats_get": (I, [H, u32, P]),
        "sg_window_nodes_top_tail": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_groups_top_tail": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_group_nodes_top_tail": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_set_traffic_trend": (I, [H, u32, P]),
        "sg_window_traffic": (I, [H, P, sz, P, sz, Psz]), "sg_window_node_traffic": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_group_traffic": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_node_traffic": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_traffic_buffer": (I, [H, u32, PP]),
        "sg_traffic_trend_entries": (I, [H, u32, P, sz, Psz]), "sg_traffic_trend_stats_get": (I, [H, u32, P]),
        "sg_window_nodes_top_traffic": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_groups_top_traffic": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_window_group_nodes_top_traffic": (I, [H, u32, u32, f32, P, P, sz, Psz, Psz]),
        "sg_set_slo": (I, [H, u32, P]), "sg_slo_assign": (I, [H, u32, P, P, sz]),
        "sg_window_node_slo": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_node_slo": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_slo_buffer": (I, [H, u32, PP]),
        "sg_slo_entries": (I, [H, u32, P, sz, Psz]), "sg_slo_stats_get": (I, [H, u32, P]),
        "sg_window_nodes_top_slo": (I, [H, u32, u32, u32, P, P, sz, Psz, Psz]),
        "sg_window_group_nodes_top_slo": (I, [H, u32, u32, u32, P, P, sz, Psz, Psz]),
        "sg_set_replicas": (I, [H, P]),
        "sg_window_replicas": (I, [H, P, sz, P, sz, Psz]), "sg_window_group_replicas": (I, [H, P, sz, P, sz, Psz]),
        "sg_window_replicas_buffer": (I, [H, PP, PP]),
        "sg_window_replicas_top": (I, [H, u32, u32, u32, P, P, sz, Psz, Psz]),
    }


#: the C ABI, once: load_library applies it to the library, EXPORTS is its names (tests/test_abi.py holds them to the header)
_SIGNATURES = _signatures()
EXPORTS = list(_SIGNATURES)


class ServiceGraphError(RuntimeError):
    def __init__(self, rc: int, msg: str):
        super().__init__(f"servicegraph rc={rc}: {msg}")
        self.rc = rc


def _rank_seed(seed) -> int:
    """sg_rank_params.seed: a name of RANK_SEED, or SG_RANK_SEED_* as it is"""
    if not isinstance(seed, str):
        return seed
    if seed not in RANK_SEED:
        raise ValueError(f"seed must be one of {sorted(RANK_SEED)}, not {seed!r}")
    return RANK_SEED[seed]


#: One row per opt-in stage that a params struct switches on (ServiceGraph._set_stage): the C function, its struct (whose fields are
#: the parameters it accepts), the defaults, the two messages' nouns, and the fields that are translated on their way into the struct.
_Stage = namedtuple("_Stage", "call struct defaults off noun convert", defaults=({},))
_STAGES = dict(
    trend=_Stage("sg_set_trend", SgTrendParams, TREND_DEFAULTS, "set_trend(None) switches the trend off", "trend"),
    node_trend=_Stage("sg_set_node_trend", SgTrendParams, TREND_DEFAULTS, "set_node_trend(None) switches the node trend off", "node trend"),
    vanished=_Stage("sg_set_vanished", SgVanishedParams, VANISHED_DEFAULTS, "set_vanished(None) switches the list off", "vanished"),
    rank=_Stage("sg_set_rank", SgRankParams, RANK_DEFAULTS, "set_rank(None) switches the ranking off", "rank", dict(seed=_rank_seed)),
    incidents=_Stage("sg_set_incidents", SgIncidentParams, INCIDENT_DEFAULTS, "set_incidents(None) switches the incidents off", "incident",
                     dict(by=lambda by: ServiceGraph._by(by) if isinstance(by, str) else by)),
    tracks=_Stage("sg_set_tracks", SgTrackParams, TRACK_DEFAULTS, "set_tracks(None) switches tracking off", "track"),
    groups=_Stage("sg_set_groups", SgGroupParams, GROUP_DEFAULTS, "set_groups(None) switches the groups off", "group",
                  dict(reserved=lambda r: (C.c_uint32 * 2)(*((r, 0) if isinstance(r, int) else tuple(r))))),
    group_trend=_Stage("sg_set_group_trend", SgTrendParams, TREND_DEFAULTS, "set_group_trend(None) switches the group trend off", "group trend"),
    group_vanished=_Stage("sg_set_group_vanished", SgVanishedParams, VANISHED_DEFAULTS, "set_group_vanished(None) switches the list off",
                          "group vanished"),
    group_node_trend=_Stage("sg_set_group_node_trend", SgTrendParams, TREND_DEFAULTS,
                            "set_group_node_trend(None) switches the workload trend off", "workload trend"),
    group_rank=_Stage("sg_set_group_rank", SgRankParams, RANK_DEFAULTS, "set_group_rank(None) switches the workload ranking off",
                      "workload rank", dict(seed=_rank_seed)),
    group_incidents=_Stage("sg_set_group_incidents", SgIncidentParams, INCIDENT_DEFAULTS,
                           "set_group_incidents(None) switches the workload incidents off", "workload incident",
                           dict(by=lambda by: ServiceGraph._by(by) if isinstance(by, str) else by)),
    group_tracks=_Stage("sg_set_group_tracks", SgTrackParams, TRACK_DEFAULTS, "set_group_tracks(None) switches workload tracking off",
                        "workload track"),
    quantile_trend=_Stage("sg_set_quantile_trend", SgTrendParams, TREND_DEFAULTS, "set_quantile_trend(params=None) switches the tail baselines off",
                          "tail trend"),
    traffic_trend=_Stage("sg_set_traffic_trend", TrafficParams, TRAFFIC_DEFAULTS, "set_traffic_trend(params=None) switches the traffic baselines off",
                         "traffic trend"),
    slo=_Stage("sg_set_slo", SloParams, SLO_DEFAULTS, "set_slo(params=None) switches the SLO stage off", "SLO"),
    replicas=_Stage("sg_set_replicas", ReplicaParams, REPLICA_DEFAULTS, "set_replicas(None) switches the replica outliers off", "replica",
                    dict(reserved=lambda r: (C.c_uint32 * 2)(*((r, 0) if isinstance(r, int) else tuple(r))))),
)

_lib = None
_lib_dev = None


def load_library(path: str = LIB_PATH, dev: bool = False) -> C.CDLL:
    """dlopen the engine.  torch is imported first so that the HIP runtime torch ships is the one
    both share (same soname, one copy per process): device pointers of torch tensors are then
    valid arguments of sg_ingest_device / the halo calls."""
    global _lib, _lib_dev
    if dev:
        if _lib_dev is not None:
            return _lib_dev
        path = os.environ.get("SG_LIB_DEV", LIB_DEV_PATH)   # (another development build: A/B runs of two kernel forms on one box)
        if path == LIB_DEV_PATH:                             # the tree's own development build: rebuilt when older than its sources
            from . import build
            build.build_engine(dev=True)
    else:
        if _lib is not None:
            return _lib
        path = os.environ.get("SG_LIB", path)          # another build of the same sources
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m alaz_amd.build` "
                           "(hipcc, gfx950). The ServiceGraph engine has no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads libamdhip64 with RTLD_GLOBAL semantics first)
    except Exception:
        pass
    # (the development build is loaded locally: it exports the same names as the shipped library and both may be loaded in one process;
    # both are linked -Bsymbolic, so neither's own calls can land in the other)
    lib = C.CDLL(path, mode=C.RTLD_LOCAL if dev else C.RTLD_GLOBAL)
    for name, (res, args) in _SIGNATURES.items():
        f = getattr(lib, name)          # AttributeError if the library does not export it
        f.restype = res; f.argtypes = args
    if dev:
        _lib_dev = lib
    else:
        _lib = lib
    return lib


class RcclComm:
    """The engine library's own RCCL communicator (sg_comm_*): rank 0 draws the unique id, `bcast(bytes) -> bytes` hands it to
    every rank (torch.distributed.broadcast_object_list, MPI, a file ...), every rank joins."""

    @staticmethod
    def probe() -> bool:
        """Can the library reach RCCL in this process?  (Agree on a fallback with every rank BEFORE constructing: a rank that fails
        inside the constructor leaves the others waiting in ncclCommInitRank.)"""
        return load_library().sg_comm_probe() == SG_OK

    def __init__(self, rank: int, world: int, device: int, bcast):
        l = load_library()
        buf = (C.c_char * 128)()
        rc = l.sg_comm_unique_id(buf, 128) if rank == 0 else SG_OK
        raw = bcast(bytes(buf.raw) if rc == SG_OK else b"")      # an empty id tells every rank that rank 0 has no RCCL: all of them raise
        if not raw:
            raise ServiceGraphError(rc if rc != SG_OK else SG_ENODEV, "sg_comm_unique_id: librccl could not be loaded on rank 0")
        idb = (C.c_char * 128).from_buffer_copy(raw)
        p = C.c_void_p()
        rc = l.sg_comm_create(idb, 128, rank, world, device, C.byref(p))
        if rc != SG_OK:
            raise ServiceGraphError(rc, "sg_comm_create (ncclCommInitRank) failed")
        self._l, self.ptr, self.rank, self.world = l, p, rank, world

    def close(self):
        if getattr(self, "ptr", None):
            self._l.sg_comm_destroy(self.ptr); self.ptr = None


def ip_u32(s: str) -> int:
    a, b, c, d = (int(x) for x in s.split("."))
    return (a << 24) | (b << 16) | (c << 8) | d


class ServiceGraph:
    """One engine handle (one GPU / one shard)."""

    def __init__(self, *, max_known_nodes: int, max_edges: int, layers: int = 1, max_labels: int = 1024,
                 max_outbound_ips: int = 1024, max_ips: int = 0, max_batch: int = 1 << 20, device: int = 0,
                 rank: int = 0, world: int = 1, k1_variant: int = 0, max_window_events: int = 0, windows_in_flight: int = 1,
                 edge_histogram: bool = False, warm: Optional[bool] = None, dev_knobs: Optional[bool] = None):
        # dev_knobs: the development build (SG_* environment knobs, SG_ABLATE, phase stamps).  None = that build when a knob is set in the
        # environment (tools/k1_sweep.py, tools/stamps.py, the A/B tests of alternative kernel paths), the shipped library otherwise.
        if dev_knobs is None:
            dev_knobs = any(k in os.environ for k in DEV_KNOBS)
        self._l = load_library(dev=dev_knobs)
        cfg = make_config(max_known_nodes=max_known_nodes, max_edges=max_edges, layers=layers, max_labels=max_labels,
                          max_outbound_ips=max_outbound_ips, max_ips=max_ips, max_batch=max_batch, device=device, rank=rank, world=world,
                          k1_variant=k1_variant, max_window_events=max_window_events, windows_in_flight=windows_in_flight,
                          flags=(CFG_EDGE_HISTOGRAM if edge_histogram else 0) | (0 if warm is None else (CFG_WARM if warm else CFG_NO_WARM)))   # warm: None = the engine's own rule
        h = C.c_void_p()
        rc = self._l.sg_create(C.byref(cfg), C.byref(h))
        if rc != SG_OK:
            raise ServiceGraphError(rc, "sg_create failed (no usable gfx950 device, or bad config); there is no CPU fallback")
        self._h = h
        self.layers = layers
        self.max_edges = max_edges
        self.max_batch = max_batch
        self.rank, self.world = rank, world

    # ---- plumbing ----
    def _ck(self, rc: int, allow=()):
        if rc != SG_OK and rc not in allow:
            raise ServiceGraphError(rc, (self._l.sg_last_error(self._h) or b"").decode())
        return rc

    def _set_stage(self, stage: str, params, kw, *lead) -> Optional[dict]:
        """every set_* with a params struct (_STAGES): call(h, *lead, NULL) for params None, else call(h, *lead, the struct filled by
        field name from the defaults, params and kw); returns the merged parameters"""
        st = _STAGES[stage]
        call = getattr(self._l, st.call)
        if params is None:
            if kw:
                raise TypeError(f"{st.off} and takes no parameters")
            self._ck(call(self._h, *lead, None))
            return None
        v = dict(st.defaults)
        v.update(params or {}); v.update(kw)
        unknown = set(v) - {f for f, _ in st.struct._fields_}
        if unknown:
            raise TypeError(f"unknown {st.noun} parameters: {sorted(unknown)}")
        p = st.struct(struct_size=C.sizeof(st.struct))
        for f, x in v.items():
            setattr(p, f, st.convert[f](x) if f in st.convert else x)
        self._ck(call(self._h, *lead, C.byref(p)))
        return v

    def _counted(self, call, dtype, shape_tail=()) -> np.ndarray:
        """two calls: call(h, NULL, 0, &n) for the count, call(h, out, n, &n) for the rows"""
        n = C.c_size_t(0)
        self._ck(call(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value,) + shape_tail, dtype=dtype)
        if n.value:
            self._ck(call(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def _window_rows(self, call, dtype, index):
        """call(h, index, n_index, out, cap, &n): every row of the last read window (index None: the count, then the rows), or those at index"""
        if index is None:
            return self._counted(lambda h, out, cap, n: call(h, None, 0, out, cap, n), dtype)
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        out = np.zeros(len(idx), dtype=dtype)
        if len(idx):
            self._ck(call(self._h, idx.ctypes.data, len(idx), out.ctypes.data, len(idx), C.byref(C.c_size_t(0))))
        return out

    def _capped(self, call, cap: Optional[int]) -> np.ndarray:
        """room for cap rows (None = max_edges), call(out, cap, &n), the min(n, cap) rows that were written"""
        cap = self.max_edges if cap is None else cap
        out = np.zeros(cap, dtype=EDGE_OUT_DTYPE); n = C.c_size_t(0)
        self._ck(call(out.ctypes.data, cap, C.byref(n)))
        return out[: min(n.value, cap)]

    def _top(self, call, cap: int, *dtypes):
        """a selection into host memory: one array of cap rows per dtype, call(*arrays, cap, &n_selected, &n_total), the
        min(n_selected, cap) rows of each that were written and n_total"""
        outs = [np.zeros(cap, dtype=d) for d in dtypes]
        ns, nt = C.c_size_t(0), C.c_size_t(0)
        self._ck(call(*[o.ctypes.data for o in outs], cap, C.byref(ns), C.byref(nt)))
        m = min(ns.value, cap)
        return (*[o[:m] for o in outs], nt.value)

    def _node_cap(self, k: int, cap: Optional[int], count=None) -> int:
        """a node selection's cap: the caller's, else k, else (k = 0) the window's node count — one count(h, NULL, 0, &n) call
        (sg_window_nodes; sg_window_group_nodes for the workload rows)"""
        if cap is not None:
            return cap
        if k:
            return k
        n = C.c_size_t(0)
        self._ck((count or self._l.sg_window_nodes)(self._h, None, 0, C.byref(n)))
        return n.value

    def _pointers(self, call, n: int) -> tuple:
        """call(h, &p0 .. &p(n-1)): the n device pointers as ints"""
        p = [C.c_void_p() for _ in range(n)]
        self._ck(call(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def _stats(self, call, struct):
        s = struct()
        self._ck(call(self._h, C.byref(s)))
        return s

    def close(self):
        if getattr(self, "_h", None):
            self._l.sg_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def geometry(self) -> dict:
        """What sg_create chose for K1 (sg_geometry_get) and, as prepare_fold, whether its warm closes launch no kc_prepare (sg_prepare_fold_get)."""
        g = SgGeometry()
        self._ck(self._l.sg_geometry_get(self._h, C.byref(g)))
        fold = C.c_uint32(0)
        self._ck(self._l.sg_prepare_fold_get(self._h, C.byref(fold)))
        pair = C.c_uint32(0)
        self._ck(self._l.sg_pass_a_pair_get(self._h, C.byref(pair)))
        form = C.c_uint32(0)
        self._ck(self._l.sg_k5_form_get(self._h, C.byref(form)))
        efeat = C.c_uint32(0)
        self._ck(self._l.sg_k5_efeat_get(self._h, C.byref(efeat)))
        k3in, k3feat = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._l.sg_k3_forms_get(self._h, C.byref(k3in), C.byref(k3feat)))
        return {**{n: int(getattr(g, n)) for n, _ in SgGeometry._fields_}, "prepare_fold": int(fold.value), "pass_a_pair": int(pair.value), "k5_form": int(form.value),
                "k5_efeat": int(efeat.value), "k3_in_form": int(k3in.value), "k3_feat_lanes": int(k3feat.value)}

    def k1_kernels(self) -> tuple:
        """Names of the two K1 kernels this engine launches (as rocprofv3 lists them), or the single global-table kernel."""
        g = self.geometry()
        if g["k1_variant"] == 1: return ("k1_resolve_aggregate",)
        if not g["k1_narrow"]: return ("k1a_partition", "k1b_merge")
        return ("k1a_team_partition" if g["pass_a_teams"] else "k1a_tile_partition", "k1b_stream_merge")

    # ---- join tables (aggregator/persist.go:55-71,114-130) ----
    def upsert_pod(self, ip: int, node_id: int): self._ck(self._l.sg_upsert_pod(self._h, ip, node_id))
    def delete_pod(self, ip: int): self._ck(self._l.sg_delete_pod(self._h, ip))
    def upsert_service(self, ip: int, node_id: int): self._ck(self._l.sg_upsert_service(self._h, ip, node_id))
    def delete_service(self, ip: int): self._ck(self._l.sg_delete_service(self._h, ip))
    def set_clock(self, first_kernel_ns: int, first_user_ns: int): self._ck(self._l.sg_set_clock(self._h, first_kernel_ns, first_user_ns))
    def set_label_count(self, n: int): self._ck(self._l.sg_set_label_count(self._h, n))

    def load_weights(self, w: np.ndarray):
        w = np.ascontiguousarray(w, dtype=np.float32)
        self._ck(self._l.sg_load_weights(self._h, w.ctypes.data, len(w)))

    # ---- ingest ----
    def ingest(self, events: np.ndarray) -> int:
        ev = np.ascontiguousarray(events)
        assert ev.dtype == EVENT_DTYPE
        return self._ck(self._l.sg_ingest(self._h, ev.ctypes.data, len(ev)), allow=(SG_EAGAIN,))

    def host_register(self, arr: np.ndarray):
        """Page-lock a (contiguous) numpy array so that ingest_pinned can read slices of it without the staging copy."""
        assert arr.flags.c_contiguous
        self._ck(self._l.sg_host_register(self._h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr: np.ndarray): self._ck(self._l.sg_host_unregister(self._h, arr.ctypes.data))

    def ingest_pinned(self, events: np.ndarray) -> int:
        """events: a slice of a registered array; it must stay unchanged until the window has been closed."""
        assert events.dtype == EVENT_DTYPE and events.flags.c_contiguous
        return self._ck(self._l.sg_ingest_pinned(self._h, events.ctypes.data, len(events)), allow=(SG_EAGAIN,))

    def ingest_bulk(self, events: np.ndarray, pinned: bool = False) -> int:
        """All of `events` in max_batch pieces, waiting for a free staging slot instead of dropping; returns the waits."""
        assert events.dtype == EVENT_DTYPE and events.flags.c_contiguous
        w = C.c_uint64(0)
        self._ck(self._l.sg_ingest_bulk(self._h, events.ctypes.data, len(events), 1 if pinned else 0, C.byref(w)))
        return int(w.value)

    def ingest_device(self, dev_ptr: int, n: int, stream: int = 0):
        self._ck(self._l.sg_ingest_device(self._h, dev_ptr, n, stream or None))

    # ---- window ----
    def flush_window(self, window_end_ms: int = 0, cap: Optional[int] = None) -> np.ndarray:
        return self._capped(lambda out, c, n: self._l.sg_flush_window(self._h, window_end_ms, out, c, n), cap)

    def flush_window_view(self, window_end_ms: int = 0) -> np.ndarray:
        """The window's rows as a read-only VIEW of the engine's page-locked host buffer (no copy): valid until the next
        flush_window / flush_window_view / window_read on this engine."""
        ptr = C.c_void_p(); n = C.c_size_t(0)
        self._ck(self._l.sg_flush_window_view(self._h, window_end_ms, C.byref(ptr), C.byref(n)))
        return self._rows_view(ptr, n)

    def flush_begin(self, window_end_ms: int = 0):
        """Close the window and enqueue its pipeline (sg_flush_begin); ingest calls from here on fill the next window."""
        self._ck(self._l.sg_flush_begin(self._h, window_end_ms))

    def flush_end_view(self) -> np.ndarray:
        """The rows of the window flush_begin closed, as flush_window_view returns them (any thread; the engine lock is not held
        while the rows are fetched)."""
        ptr = C.c_void_p(); n = C.c_size_t(0)
        self._ck(self._l.sg_flush_end_view(self._h, C.byref(ptr), C.byref(n)))
        return self._rows_view(ptr, n)

    def flush_end(self, cap: int | None = None) -> np.ndarray:
        return self._capped(lambda out, c, n: self._l.sg_flush_end(self._h, out, c, n), cap)

    # ---- selection (K7): only the selected rows leave the device ----
    @staticmethod
    def _by(by) -> int:
        if by not in SEL_BY:
            raise ValueError(f"by must be one of {sorted(SEL_BY)}, not {by!r}")
        return SEL_BY[by]

    def flush_window_top(self, k: int, min_score: float = float("-inf"), window_end_ms: int = 0, cap: Optional[int] = None,
                         by: str = "score"):
        """Close the window and return (rows, row_index, n_edges) of its selection (sg_flush_window_top): k = 0 every row with
        score >= min_score in canonical order, else the k highest-scoring such rows, descending, ties by row position.  cap
        defaults to k (k > 0) or max_edges; rows beyond it are counted, not returned.  by = "lat_dev" / "err_dev" / "new" selects
        by the row's trend instead of its score (sg_flush_window_top_by; min_score is then the threshold on that value)."""
        b = self._by(by)
        cap = (k or self.max_edges) if cap is None else cap
        if b:
            return self._top(lambda *a: self._l.sg_flush_window_top_by(self._h, window_end_ms, b, k, min_score, *a), cap, EDGE_OUT_DTYPE, np.uint32)
        return self._top(lambda *a: self._l.sg_flush_window_top(self._h, window_end_ms, k, min_score, *a), cap, EDGE_OUT_DTYPE, np.uint32)

    def flush_end_top(self, k: int, min_score: float = float("-inf"), cap: Optional[int] = None, by: str = "score"):
        """flush_window_top for the window flush_begin closed (sg_flush_end_top / sg_flush_end_top_by)."""
        b = self._by(by)
        cap = (k or self.max_edges) if cap is None else cap
        if b:
            return self._top(lambda *a: self._l.sg_flush_end_top_by(self._h, b, k, min_score, *a), cap, EDGE_OUT_DTYPE, np.uint32)
        return self._top(lambda *a: self._l.sg_flush_end_top(self._h, k, min_score, *a), cap, EDGE_OUT_DTYPE, np.uint32)

    def window_select(self, k: int, min_score: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0, by: str = "score"):
        """Select from the rows of the window window_run closed last into device memory (sg_window_select): d_out [cap] rows,
        d_index [cap] u32 (0 = none), d_n one u64 = rows selected; enqueued on `stream` (0 = that window's stream).  by as in
        flush_window_top (sg_window_select_by: that window's trend rows)."""
        b = self._by(by)
        if b:
            self._ck(self._l.sg_window_select_by(self._h, b, k, min_score, d_out or None, d_index or None, cap, d_n, stream or None))
        else:
            self._ck(self._l.sg_window_select(self._h, k, min_score, d_out or None, d_index or None, cap, d_n, stream or None))

    # ---- per-edge baselines (K8): each edge against its own past ----
    def set_trend(self, params: Optional[dict] = (), **kw):
        """Switch the per-edge baseline on (sg_set_trend; shift, warmup, ttl, max_entries, lat_floor_ns, err_floor as keywords or a
        dict — see TREND_DEFAULTS; set_trend() = every default; (re)enabling starts an empty baseline) or off: set_trend(None)."""
        v = self._set_stage("trend", params, kw)
        if v is not None:
            self._trend_entries = v["max_entries"] or min(1 << 31, 2 * max(self.max_edges, 1))   # the baseline's capacity

    def window_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """TREND_DTYPE rows of the last read window (sg_window_trend): every row, or the rows at `index` (only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_trend, TREND_DTYPE, index)

    def trend_buffer(self) -> int:
        """device pointer of the sg_edge_trend rows of the window window_run closed last (sg_window_trend_buffer)"""
        return self._pointers(self._l.sg_window_trend_buffer, 1)[0]

    def trend_entries(self) -> np.ndarray:
        """the baseline in key order, TREND_ENTRY_DTYPE (sg_trend_entries)"""
        return self._counted(self._l.sg_trend_entries, TREND_ENTRY_DTYPE)

    def trend_stats(self) -> SgTrendStats:
        return self._stats(self._l.sg_trend_stats_get, SgTrendStats)

    def set_vanished(self, params: Optional[dict] = (), **kw):
        """Switch K8's vanished list on (sg_set_vanished; silent_windows, min_seen, max_rows as keywords or a dict — see
        VANISHED_DEFAULTS; needs the trend on) or off: set_vanished(None).  Any set_trend call switches it off."""
        v = self._set_stage("vanished", params, kw)
        if v is not None:
            self._van_rows = v["max_rows"] or min(65536, self._trend_entries)   # (the rows a window's list holds at most)

    def window_vanished(self, with_count: bool = False):
        """VANISHED_DTYPE list of the last read window (sg_window_vanished), ascending by edge key; with_count: (list, count of
        every vanished entry of the window, which may exceed max_rows)."""
        out = self._counted(self._l.sg_window_vanished, VANISHED_DTYPE)       # (room for the count; max_rows of them are written)
        rows = out[: self._van_rows]
        return (rows, len(out)) if with_count else rows

    def vanished_buffer(self) -> Tuple[int, int]:
        """(device pointer of the sg_edge_vanished list, device pointer of its u64 count) of the window window_run closed last
        (sg_window_vanished_buffer)"""
        return self._pointers(self._l.sg_window_vanished_buffer, 2)

    # ---- node rollup (K9): each window's rows reduced per node on the device ----
    def set_nodes(self, on: bool = True):
        """Switch the per-window node rollup on (sg_set_nodes: allocates its buffers) or off (frees them)."""
        self._ck(self._l.sg_set_nodes(self._h, 1 if on else 0))

    def window_nodes(self) -> np.ndarray:
        """NODE_DTYPE rows of the last read window (sg_window_nodes), ascending by (ref type, ref value)"""
        return self._counted(self._l.sg_window_nodes, NODE_DTYPE)

    def nodes_buffer(self) -> Tuple[int, int]:
        """(device pointer of the sg_node_out rows, device pointer of their u64 count) of the window window_run closed last
        (sg_window_nodes_buffer)"""
        return self._pointers(self._l.sg_window_nodes_buffer, 2)

    # ---- node baselines (K10) and node selection: each service against its own past ----
    def set_node_trend(self, params: Optional[dict] = (), **kw):
        """Switch the per-node baseline on (sg_set_node_trend; the parameters of set_trend, max_entries 0 = 4 x the node capacity;
        needs the node rollup on; (re)enabling starts an empty baseline) or off: set_node_trend(None)."""
        self._set_stage("node_trend", params, kw)

    def window_node_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE rows of the last read window (sg_window_node_trend), row k for node row k of window_nodes(); or the rows
        of the nodes at `index` (window_nodes_top's indices; only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_node_trend, NODE_TREND_DTYPE, index)

    def node_trend_buffer(self) -> int:
        """device pointer of the sg_node_trend rows of the window window_run closed last (sg_window_node_trend_buffer)"""
        return self._pointers(self._l.sg_window_node_trend_buffer, 1)[0]

    def node_trend_entries(self) -> np.ndarray:
        """the node baseline in key order, TREND_ENTRY_DTYPE with to_key = side (0 in, 1 out) (sg_node_trend_entries)"""
        return self._counted(self._l.sg_node_trend_entries, TREND_ENTRY_DTYPE)

    def node_trend_stats(self) -> SgTrendStats:
        return self._stats(self._l.sg_node_trend_stats_get, SgTrendStats)

    @staticmethod
    def _nby(by) -> int:
        if by not in NSEL_BY:
            raise ValueError(f"by must be one of {sorted(NSEL_BY)}, not {by!r}")
        return NSEL_BY[by]

    def window_nodes_top(self, k: int, min_value: float = float("-inf"), by: str = "score", cap: Optional[int] = None):
        """(node rows, node indices, n_nodes) of a selection over the last read window's node rows (sg_window_nodes_top): k = 0
        every node with value >= min_value in node order, else the k highest such, descending, ties by node position.  by: a key
        of NSEL_BY.  cap defaults to k (k > 0) or the window's node count; nodes beyond it are counted, not returned."""
        b = self._nby(by)
        return self._top(lambda *a: self._l.sg_window_nodes_top(self._h, b, k, min_value, *a), self._node_cap(k, cap), NODE_DTYPE, np.uint32)

    def window_nodes_select(self, k: int, min_value: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0,
                            by: str = "score"):
        """Select from the node rows of the window window_run closed last into device memory (sg_window_nodes_select): d_out
        [cap] node rows (0 = none), d_index [cap] u32 (0 = none), d_n one u64 = nodes selected; enqueued on `stream` (0 = that
        window's stream)."""
        self._ck(self._l.sg_window_nodes_select(self._h, self._nby(by), k, min_value, d_out or None, d_index or None, cap, d_n,
                                                stream or None))

    # ---- culprit ranking (K11): a walk over the window's own graph, mass piling up where the anomalous rows stop ----
    def set_rank(self, params: Optional[dict] = (), **kw):
        """Switch the per-window culprit ranking on (sg_set_rank; iters, damping_q8, seed ("score" / "uniform" or SG_RANK_SEED_*),
        seed_min_score as keywords or a dict — see RANK_DEFAULTS; needs the node rollup on) or off: set_rank(None)."""
        self._set_stage("rank", params, kw)

    def window_rank(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """RANK_DTYPE rows of the last read window (sg_window_rank), row k for node row k of window_nodes(); or the rows of the
        nodes at `index` (only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_rank, RANK_DTYPE, index)

    def rank_buffer(self) -> int:
        """device pointer of the sg_node_rank rows of the window window_run closed last (sg_window_rank_buffer)"""
        return self._pointers(self._l.sg_window_rank_buffer, 1)[0]

    def window_rank_top(self, k: int, min_share: float = float("-inf"), cap: Optional[int] = None):
        """(node rows, rank rows, node indices, n_nodes) of a selection over the last read window's rank rows
        (sg_window_rank_top): k = 0 every node with rank >= 2^24 and share >= min_share in node order, else the k highest such,
        descending, ties by node position.  cap defaults to k (k > 0) or the window's node count."""
        return self._top(lambda *a: self._l.sg_window_rank_top(self._h, k, min_share, *a), self._node_cap(k, cap),
                         NODE_DTYPE, RANK_DTYPE, np.uint32)

    def window_rank_select(self, k: int, min_share: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0):
        """Select from the rank rows of the window window_run closed last into device memory (sg_window_rank_select): d_out [cap]
        node rows (0 = none), d_index [cap] u32 (0 = none), d_n one u64 = nodes selected; enqueued on `stream` (0 = that window's
        stream)."""
        self._ck(self._l.sg_window_rank_select(self._h, k, min_share, d_out or None, d_index or None, cap, d_n, stream or None))

    # ---- incidents (K12): the window's red rows grouped into connected components ----
    def set_incidents(self, params: Optional[dict] = (), **kw):
        """Switch the per-window incident grouping on (sg_set_incidents; by = "score" / "lat_dev" / "err_dev" or SG_SEL_*, min_value
        as keywords or a dict; needs the node rollup on, and the trend for a trend key) or off: set_incidents(None)."""
        self._set_stage("incidents", params, kw)

    def window_incidents(self) -> np.ndarray:
        """INCIDENT_DTYPE rows of the last read window (sg_window_incidents), numbered by their smallest node row"""
        return self._counted(self._l.sg_window_incidents, INCIDENT_DTYPE)

    def window_node_incident(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """the incident number (NO_INCIDENT: none) of every node row of the last read window (sg_window_node_incident), or of the
        nodes at `index`"""
        return self._window_rows(self._l.sg_window_node_incident, np.dtype("<u4"), index)

    def window_incidents_buffer(self) -> Tuple[int, int, int]:
        """(device pointer of the sg_incident_out rows, of their u64 count, of the u32 incident per node row) of the window
        window_run closed last (sg_window_incidents_buffer)"""
        return self._pointers(self._l.sg_window_incidents_buffer, 3)

    # ---- tracks (K13): the incidents followed across windows ----
    def set_tracks(self, params: Optional[dict] = (), **kw):
        """Switch the tracking of incidents across windows on (sg_set_tracks; quiet_windows (default 2), max_tracks (0 = never cut)
        as keywords or a dict; needs the incidents on) or off: set_tracks(None).  Any set_incidents call switches it off."""
        self._set_stage("tracks", params, kw)

    def window_incident_tracks(self) -> np.ndarray:
        """TRACK_DTYPE rows of the last read window (sg_window_incident_tracks): row i is the track of window_incidents()[i]"""
        return self._counted(self._l.sg_window_incident_tracks, TRACK_DTYPE)

    def window_tracks_ended(self) -> np.ndarray:
        """TRACK_ENTRY_DTYPE entries of the tracks that went quiet in the last read window (sg_window_tracks_ended), in id order"""
        return self._counted(self._l.sg_window_tracks_ended, TRACK_ENTRY_DTYPE)

    def window_tracks_buffer(self) -> Tuple[int, int, int]:
        """(device pointer of the sg_incident_track rows, of the ended sg_track_entry list, of its u64 count) of the window
        window_run closed last (sg_window_tracks_buffer)"""
        return self._pointers(self._l.sg_window_tracks_buffer, 3)

    def track_entries(self) -> np.ndarray:
        """the live track table in id order, TRACK_ENTRY_DTYPE (sg_track_entries)"""
        return self._counted(self._l.sg_track_entries, TRACK_ENTRY_DTYPE)

    def track_stats(self) -> SgTrackStats:
        return self._stats(self._l.sg_track_stats_get, SgTrackStats)

    # ---- groups (K14): the window's service map contracted to workloads ----
    def set_groups(self, params: Optional[dict] = (), **kw):
        """Switch the per-window contraction to workloads on (sg_set_groups; max_groups (0 = max_known_nodes) as a keyword or a
        dict; needs no other stage) or off: set_groups(None).  Every call starts from a map with nothing grouped."""
        self._set_stage("groups", params, kw)

    def group_assign(self, node_ids, groups):
        """group[node_ids[i]] = groups[i] (sg_group_assign; NO_GROUP takes a node out of its group).  The windows closed from now
        on are contracted under the new map."""
        ids = np.ascontiguousarray(node_ids, dtype=np.uint32)
        gs = np.ascontiguousarray(np.broadcast_to(np.asarray(groups, dtype=np.uint32), ids.shape))
        self._ck(self._l.sg_group_assign(self._h, ids.ctypes.data, gs.ctypes.data, len(ids)))

    def window_groups(self) -> np.ndarray:
        """GROUP_EDGE_DTYPE rows of the last read window (sg_window_groups), ascending by (group key of from, group key of to)"""
        return self._counted(self._l.sg_window_groups, GROUP_EDGE_DTYPE)

    def window_row_group(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """the group edge of every row of the last read window (sg_window_row_group), or of the rows at `index` (gathered on the
        device)"""
        return self._window_rows(self._l.sg_window_row_group, np.dtype("<u4"), index)

    def window_group_perm(self) -> np.ndarray:
        """the rows of the last read window in group order (sg_window_group_perm): row indices, u32"""
        return self._counted(self._l.sg_window_group_perm, np.dtype("<u4"))

    def window_groups_buffer(self) -> Tuple[int, int, int, int]:
        """(device pointer of the sg_group_edge rows, of their u64 count, of the u32 row_group, of the u32 perm) of the window
        window_run closed last (sg_window_groups_buffer)"""
        return self._pointers(self._l.sg_window_groups_buffer, 4)

    # ---- workload baselines (K15): each group edge against its own past; they survive a rollout, the pod-level ones do not ----
    def set_group_trend(self, params: Optional[dict] = (), **kw):
        """Switch the per-workload-edge baseline on (sg_set_group_trend; the parameters of set_trend; needs the groups on;
        (re)enabling starts an empty baseline) or off: set_group_trend(None).  Any set_groups call switches it off."""
        v = self._set_stage("group_trend", params, kw)
        if v is not None:
            self._gtrend_entries = v["max_entries"] or min(1 << 31, 2 * max(self.max_edges, 1))   # the baseline's capacity

    def window_group_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """TREND_DTYPE rows of the last read window (sg_window_group_trend), row k for group edge k of window_groups(); or the rows
        of the group edges at `index` (window_groups_top's indices; only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_group_trend, TREND_DTYPE, index)

    def window_group_trend_buffer(self) -> int:
        """device pointer of the group trend rows of the window window_run closed last (sg_window_group_trend_buffer)"""
        return self._pointers(self._l.sg_window_group_trend_buffer, 1)[0]

    def group_trend_entries(self) -> np.ndarray:
        """the workload baseline in key order, TREND_ENTRY_DTYPE with workload keys (sg_group_trend_entries)"""
        return self._counted(self._l.sg_group_trend_entries, TREND_ENTRY_DTYPE)

    def group_trend_stats(self) -> SgTrendStats:
        return self._stats(self._l.sg_group_trend_stats_get, SgTrendStats)

    def set_group_vanished(self, params: Optional[dict] = (), **kw):
        """Switch the list of vanished workload dependencies on (sg_set_group_vanished; the parameters of set_vanished; needs the
        group trend on) or off: set_group_vanished(None).  Any set_group_trend call switches it off."""
        v = self._set_stage("group_vanished", params, kw)
        if v is not None:
            self._gvan_rows = v["max_rows"] or min(65536, self._gtrend_entries)   # (the rows a window's list holds at most)

    def window_group_vanished(self, with_count: bool = False):
        """VANISHED_DTYPE list of the last read window (sg_window_group_vanished), ascending by workload key pair; with_count:
        (list, count of every vanished entry of the window, which may exceed max_rows)."""
        out = self._counted(self._l.sg_window_group_vanished, VANISHED_DTYPE)  # (room for the count; max_rows of them are written)
        rows = out[: self._gvan_rows]
        return (rows, len(out)) if with_count else rows

    def window_group_vanished_buffer(self) -> Tuple[int, int]:
        """(device pointer of the sg_edge_vanished list, of its u64 count) of the window window_run closed last
        (sg_window_group_vanished_buffer)"""
        return self._pointers(self._l.sg_window_group_vanished_buffer, 2)

    def window_groups_top(self, k: int, min_value: float = float("-inf"), by: str = "score", cap: Optional[int] = None):
        """(group edges, group-edge indices, n_groups) of a selection over the last read window's group edges
        (sg_window_groups_top): k = 0 every group edge with value >= min_value in group-edge order, else the k highest such,
        descending, ties by position.  by: a key of SEL_BY (score = score_max).  cap defaults to k (k > 0) or max_edges."""
        b = self._by(by)
        cap = (k or self.max_edges) if cap is None else cap
        return self._top(lambda *a: self._l.sg_window_groups_top(self._h, b, k, min_value, *a), cap, GROUP_EDGE_DTYPE, np.uint32)

    def window_groups_select(self, k: int, min_value: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0,
                             by: str = "score"):
        """Select from the group edges of the window window_run closed last into device memory (sg_window_groups_select): d_out
        [cap] group edges (0 = none), d_index [cap] u32 (0 = none), d_n one u64 = group edges selected; enqueued on `stream` (0 =
        that window's stream)."""
        self._ck(self._l.sg_window_groups_select(self._h, self._by(by), k, min_value, d_out or None, d_index or None, cap, d_n,
                                                 stream or None))

    # ---- workload rows (K16): the group edges rolled up per workload, their baselines and selection ----
    def set_group_nodes(self, on: bool = True):
        """Switch the per-window workload rows on (sg_set_group_nodes: allocates its buffers; needs the groups on) or off (frees them
        and the workload trend).  Any set_groups call switches them off."""
        self._ck(self._l.sg_set_group_nodes(self._h, 1 if on else 0))

    def window_group_nodes(self) -> np.ndarray:
        """NODE_DTYPE rows of the last read window (sg_window_group_nodes), one per workload, ascending by group key: the groups by
        id, then the ungrouped KNOWN nodes, LABEL, OBIP — not by the raw ref word"""
        return self._counted(self._l.sg_window_group_nodes, NODE_DTYPE)

    def window_group_nodes_buffer(self) -> Tuple[int, int]:
        """(device pointer of the sg_node_out workload rows, of their u64 count) of the window window_run closed last
        (sg_window_group_nodes_buffer)"""
        return self._pointers(self._l.sg_window_group_nodes_buffer, 2)

    def set_group_node_trend(self, params: Optional[dict] = (), **kw):
        """Switch the per-workload baseline on (sg_set_group_node_trend; the parameters of set_trend, max_entries 0 = 4 x the row
        capacity; needs the workload rows on; (re)enabling starts an empty baseline) or off: set_group_node_trend(None)."""
        self._set_stage("group_node_trend", params, kw)

    def window_group_node_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE rows of the last read window (sg_window_group_node_trend), row k for row k of window_group_nodes(); or
        the rows at `index` (window_group_nodes_top's indices; only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_group_node_trend, NODE_TREND_DTYPE, index)

    def window_group_node_trend_buffer(self) -> int:
        """device pointer of the workload trend rows of the window window_run closed last (sg_window_group_node_trend_buffer)"""
        return self._pointers(self._l.sg_window_group_node_trend_buffer, 1)[0]

    def group_node_trend_entries(self) -> np.ndarray:
        """the workload baseline in key order, TREND_ENTRY_DTYPE with from_key = the workload key, to_key = side (0 in, 1 out)
        (sg_group_node_trend_entries)"""
        return self._counted(self._l.sg_group_node_trend_entries, TREND_ENTRY_DTYPE)

    def group_node_trend_stats(self) -> SgTrendStats:
        return self._stats(self._l.sg_group_node_trend_stats_get, SgTrendStats)

    def window_group_nodes_top(self, k: int, min_value: float = float("-inf"), by: str = "score", cap: Optional[int] = None):
        """(workload rows, row indices, n_nodes) of a selection over the last read window's workload rows
        (sg_window_group_nodes_top): window_nodes_top with "node row" read as "workload row".  by: a key of NSEL_BY.  cap defaults
        to k (k > 0) or the window's row count."""
        b = self._nby(by)
        return self._top(lambda *a: self._l.sg_window_group_nodes_top(self._h, b, k, min_value, *a),
                         self._node_cap(k, cap, self._l.sg_window_group_nodes), NODE_DTYPE, np.uint32)

    def window_group_nodes_select(self, k: int, min_value: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0,
                                  by: str = "score"):
        """Select from the workload rows of the window window_run closed last into device memory (sg_window_group_nodes_select):
        d_out [cap] rows (0 = none), d_index [cap] u32 (0 = none), d_n one u64 = rows selected; enqueued on `stream` (0 = that
        window's stream)."""
        self._ck(self._l.sg_window_group_nodes_select(self._h, self._nby(by), k, min_value, d_out or None, d_index or None, cap, d_n,
                                                      stream or None))

    # ---- workload ranking (K17): K11's walk over the group edges and the workload rows ----
    def set_group_rank(self, params: Optional[dict] = (), **kw):
        """Switch the per-window workload ranking on (sg_set_group_rank; set_rank's parameters — see RANK_DEFAULTS; needs the workload
        rows on; independent of set_rank) or off: set_group_rank(None)."""
        self._set_stage("group_rank", params, kw)

    def window_group_rank(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """RANK_DTYPE rows of the last read window (sg_window_group_rank), row k for row k of window_group_nodes(); or the rows at
        `index` (only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_group_rank, RANK_DTYPE, index)

    def window_group_rank_buffer(self) -> int:
        """device pointer of the workload rank rows of the window window_run closed last (sg_window_group_rank_buffer)"""
        return self._pointers(self._l.sg_window_group_rank_buffer, 1)[0]

    def window_group_rank_top(self, k: int, min_share: float = float("-inf"), cap: Optional[int] = None):
        """(workload rows, rank rows, row indices, n_nodes) of a selection over the last read window's workload rank rows
        (sg_window_group_rank_top): window_rank_top with "node row" read as "workload row".  cap defaults to k (k > 0) or the
        window's row count."""
        return self._top(lambda *a: self._l.sg_window_group_rank_top(self._h, k, min_share, *a),
                         self._node_cap(k, cap, self._l.sg_window_group_nodes), NODE_DTYPE, RANK_DTYPE, np.uint32)

    def window_group_rank_select(self, k: int, min_share: float, d_out: int, d_index: int, cap: int, d_n: int, stream: int = 0):
        """Select from the workload rank rows of the window window_run closed last into device memory
        (sg_window_group_rank_select): d_out [cap] workload rows (0 = none), d_index [cap] u32 (0 = none), d_n one u64 = rows
        selected; enqueued on `stream` (0 = that window's stream)."""
        self._ck(self._l.sg_window_group_rank_select(self._h, k, min_share, d_out or None, d_index or None, cap, d_n, stream or None))

    # ---- workload incidents (K18): the window's red group edges grouped into connected components of workload rows ----
    def set_group_incidents(self, params: Optional[dict] = (), **kw):
        """Switch the per-window workload incident grouping on (sg_set_group_incidents; set_incidents' parameters: by = "score" /
        "lat_dev" / "err_dev" or SG_SEL_*, min_value; needs the workload rows on, and the group trend for a trend key; independent
        of set_incidents) or off: set_group_incidents(None)."""
        self._set_stage("group_incidents", params, kw)

    def window_group_incidents(self) -> np.ndarray:
        """INCIDENT_DTYPE rows of the last read window (sg_window_group_incidents), numbered by their smallest workload row; the node
        fields index window_group_nodes(), worst_row indexes window_groups()"""
        return self._counted(self._l.sg_window_group_incidents, INCIDENT_DTYPE)

    def window_group_node_incident(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """the incident number (NO_INCIDENT: none) of every workload row of the last read window (sg_window_group_node_incident), or
        of the rows at `index` (only those cross PCIe)"""
        return self._window_rows(self._l.sg_window_group_node_incident, np.dtype("<u4"), index)

    def window_group_incidents_buffer(self) -> Tuple[int, int, int]:
        """(device pointer of the sg_incident_out rows, of their u64 count, of the u32 incident per workload row) of the window
        window_run closed last (sg_window_group_incidents_buffer)"""
        return self._pointers(self._l.sg_window_group_incidents_buffer, 3)

    # ---- workload tracks (K19): the workload incidents followed across windows ----
    def set_group_tracks(self, params: Optional[dict] = (), **kw):
        """Switch the tracking of workload incidents across windows on (sg_set_group_tracks; set_tracks' parameters: quiet_windows
        (default 2), max_tracks (0 = never cut); needs the workload incidents on; independent of set_tracks) or off:
        set_group_tracks(None).  Any set_group_incidents call switches it off."""
        self._set_stage("group_tracks", params, kw)

    def window_group_incident_tracks(self) -> np.ndarray:
        """TRACK_DTYPE rows of the last read window (sg_window_group_incident_tracks): row i is the track of
        window_group_incidents()[i]"""
        return self._counted(self._l.sg_window_group_incident_tracks, TRACK_DTYPE)

    def window_group_tracks_ended(self) -> np.ndarray:
        """TRACK_ENTRY_DTYPE entries of the workload tracks that went quiet in the last read window (sg_window_group_tracks_ended),
        in id order"""
        return self._counted(self._l.sg_window_group_tracks_ended, TRACK_ENTRY_DTYPE)

    def window_group_tracks_buffer(self) -> Tuple[int, int, int]:
        """(device pointer of the sg_incident_track rows, of the ended sg_track_entry list, of its u64 count) of the window
        window_run closed last (sg_window_group_tracks_buffer)"""
        return self._pointers(self._l.sg_window_group_tracks_buffer, 3)

    def group_track_entries(self) -> np.ndarray:
        """the live workload track table in id order, TRACK_ENTRY_DTYPE (sg_group_track_entries)"""
        return self._counted(self._l.sg_group_track_entries, TRACK_ENTRY_DTYPE)

    def group_track_stats(self) -> SgTrackStats:
        return self._stats(self._l.sg_group_track_stats_get, SgTrackStats)

    # ---- workload impact (K22): who depends on each workload incident ----
    def set_group_impact(self, max_incidents: Optional[int] = 256, max_hops: int = 8):
        """Switch the per-window upstream impact of the workload incidents on (sg_set_group_impact: the first max_incidents
        incidents are covered, 1 .. IMPACT_MAX_INCIDENTS; the search is cut at max_hops call edges, 1 .. IMPACT_MAX_HOPS; needs the
        workload incidents on) or off: set_group_impact(None).  Any set_group_incidents call switches it off."""
        if max_incidents is None:
            max_incidents, max_hops = 0, 0
        self._ck(self._l.sg_set_group_impact(self._h, max_incidents, max_hops))

    def window_group_impact(self) -> np.ndarray:
        """the impact rows of the last read window (sg_window_group_impact), (n, IMPACT_WORDS) <u8: row i belongs to
        window_group_incidents()[i], the words are IMPACT_FIELDS"""
        return self._counted(self._l.sg_window_group_impact, np.dtype("<u8"), (IMPACT_WORDS,))

    def window_group_node_hops(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """the fewest call edges from every workload row of the last read window to a covered incident (0: a member; NO_HOPS: none
        within max_hops; sg_window_group_node_hops), or of the rows at index"""
        return self._window_rows(self._l.sg_window_group_node_hops, np.dtype("<u4"), index)

    def window_group_impact_mask(self) -> np.ndarray:
        """the mask rows of the last read window (sg_window_group_impact_mask), (workload rows, W) <u8: bit b of word w of row v is
        set iff incident 64 w + b is covered and reaches v within max_hops (its members included)"""
        n, w = C.c_size_t(0), C.c_uint32(0)
        self._ck(self._l.sg_window_group_impact_mask(self._h, None, 0, C.byref(n), C.byref(w)))
        out = np.zeros((n.value, w.value), dtype=np.dtype("<u8"))
        if n.value:
            self._ck(self._l.sg_window_group_impact_mask(self._h, out.ctypes.data, n.value, C.byref(n), C.byref(w)))
        return out[: n.value]

    def window_group_impact_buffer(self) -> Tuple[int, int, int, int]:
        """(device pointer of the impact rows, of their u64 count, of the u32 hops per workload row, of the mask rows) of the window
        window_run closed last (sg_window_group_impact_buffer)"""
        return self._pointers(self._l.sg_window_group_impact_buffer, 4)

    # ---- latency percentiles (K20): histograms and percentiles per node row, group edge and workload row ----
    def set_quantiles(self, spaces=("nodes",), permille=(500, 990)):
        """Switch the per-window latency histograms and percentiles on (sg_set_quantiles; the engine was created with
        edge_histogram=True): spaces is an iterable of "nodes" / "groups" / "group_nodes" (each needs its base stage on:
        set_nodes / set_groups / set_group_nodes) or the SG_Q_* bits as an int; permille up to Q_MAX values in 1 .. 1000.
        set_quantiles(None) or spaces=0 switches the stage off."""
        bits = 0 if spaces is None else spaces if isinstance(spaces, int) else self._qbits(spaces)
        qm = np.ascontiguousarray(permille, dtype=np.uint32)
        self._ck(self._l.sg_set_quantiles(self._h, bits, qm.ctypes.data if len(qm) else None, len(qm)))
        self._n_q = len(qm) if len(qm) else 2

    @staticmethod
    def _qbits(spaces) -> int:
        bits = 0
        for sp in ([spaces] if isinstance(spaces, str) else spaces):
            if sp not in Q_SPACES:
                raise ValueError(f"unknown quantile space {sp!r}: one of {sorted(Q_SPACES)}")
            bits |= Q_SPACES[sp]
        return bits

    def _quantile_dtype(self, sides: int) -> np.dtype:
        return np.dtype(("<u4", (sides, getattr(self, "_n_q", 2)) if sides == 2 else (getattr(self, "_n_q", 2),)))

    def window_node_hist(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 2, 16) u64 bins of the last read window (sg_window_node_hist): entry k for row k of window_nodes(), out side then in
        side; or the entries at `index` (only those cross PCIe)."""
        return self._window_rows(self._l.sg_window_node_hist, np.dtype(("<u8", (2, 16))), index)

    def window_node_quantiles(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 2, n_q) u32 microseconds (sg_window_node_quantiles), in set_quantiles' permille order"""
        return self._window_rows(self._l.sg_window_node_quantiles, self._quantile_dtype(2), index)

    def window_group_hist(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 16) u64 bins (sg_window_group_hist): entry k for group edge k of window_groups()"""
        return self._window_rows(self._l.sg_window_group_hist, np.dtype(("<u8", (16,))), index)

    def window_group_quantiles(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, n_q) u32 microseconds (sg_window_group_quantiles)"""
        return self._window_rows(self._l.sg_window_group_quantiles, self._quantile_dtype(1), index)

    def window_group_node_hist(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 2, 16) u64 bins (sg_window_group_node_hist): entry k for row k of window_group_nodes()"""
        return self._window_rows(self._l.sg_window_group_node_hist, np.dtype(("<u8", (2, 16))), index)

    def window_group_node_quantiles(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 2, n_q) u32 microseconds (sg_window_group_node_quantiles)"""
        return self._window_rows(self._l.sg_window_group_node_quantiles, self._quantile_dtype(2), index)

    def window_quantiles_buffer(self, space) -> Tuple[int, int]:
        """(device pointer of the u64 histograms, of the u32 quantiles — Q_MAX words an entity and side) of one space of the window
        window_run closed last (sg_window_quantiles_buffer)"""
        bits = space if isinstance(space, int) else self._qbits(space)
        return self._pointers(lambda h, *a: self._l.sg_window_quantiles_buffer(h, bits, *a), 2)

    # ---- tail baselines (K21): each entity's tracked quantile against its own past ----
    def set_quantile_trend(self, spaces=("nodes",), permille: int = 990, params: Optional[dict] = (), **kw):
        """Switch the tail baselines on (sg_set_quantile_trend): a baseline of the `permille` quantile — one of those set_quantiles
        was last given — per space, each among the spaces set_quantiles has on ("nodes" / "groups" / "group_nodes", or the SG_Q_*
        bits as an int); the parameters of set_trend as keywords or a dict, max_entries 0 = the default of the mean baseline of
        each space.  Every call starts empty baselines.  spaces None / 0 or params=None switches the stage off; so does any
        set_quantiles call."""
        bits = 0 if spaces is None else spaces if isinstance(spaces, int) else self._qbits(spaces)
        self._set_stage("quantile_trend", params, kw, bits, int(permille))

    def _qbit(self, space) -> int:
        return space if isinstance(space, int) else self._qbits(space)

    def window_node_quantile_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE tail rows of the last read window (sg_window_node_quantile_trend), row k for node row k of
        window_nodes(): lat_dev and base_mean_us of the tracked quantile, err_dev as the node trend's; or the rows at `index`."""
        return self._window_rows(self._l.sg_window_node_quantile_trend, NODE_TREND_DTYPE, index)

    def window_group_quantile_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """TREND_DTYPE tail rows (sg_window_group_quantile_trend), row k for group edge k of window_groups(); or those at `index`."""
        return self._window_rows(self._l.sg_window_group_quantile_trend, TREND_DTYPE, index)

    def window_group_node_quantile_trend(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE tail rows (sg_window_group_node_quantile_trend), row k for row k of window_group_nodes(); or those at `index`."""
        return self._window_rows(self._l.sg_window_group_node_quantile_trend, NODE_TREND_DTYPE, index)

    def window_quantile_trend_buffer(self, space) -> int:
        """device pointer of the tail rows of one space of the window window_run closed last (sg_window_quantile_trend_buffer)"""
        bits = self._qbit(space)
        return self._pointers(lambda h, *a: self._l.sg_window_quantile_trend_buffer(h, bits, *a), 1)[0]

    def quantile_trend_entries(self, space) -> np.ndarray:
        """the tail baseline of one space in key order, TREND_ENTRY_DTYPE with the keys of the mean baseline of that space and
        lat_mean / lat_dev of the tracked quantile in ns (sg_quantile_trend_entries)"""
        bits = self._qbit(space)
        return self._counted(lambda h, *a: self._l.sg_quantile_trend_entries(h, bits, *a), TREND_ENTRY_DTYPE)

    def quantile_trend_stats(self, space) -> SgTrendStats:
        bits = self._qbit(space)
        return self._stats(lambda h, *a: self._l.sg_quantile_trend_stats_get(h, bits, *a), SgTrendStats)

    def window_nodes_top_tail(self, k: int, min_value: float = float("-inf"), by: str = "in_lat_dev", cap: Optional[int] = None):
        """window_nodes_top with the tail rows as the trend source (sg_window_nodes_top_tail): by "in_lat_dev" ranks the in side's
        deviation of the tracked quantile, and so on through NSEL_BY."""
        b = self._nby(by)
        return self._top(lambda *a: self._l.sg_window_nodes_top_tail(self._h, b, k, min_value, *a), self._node_cap(k, cap), NODE_DTYPE, np.uint32)

    def window_groups_top_tail(self, k: int, min_value: float = float("-inf"), by: str = "lat_dev", cap: Optional[int] = None):
        """window_groups_top with the tail rows as the trend source (sg_window_groups_top_tail); by: a key of SEL_BY."""
        b = self._by(by)
        cap = (k or self.max_edges) if cap is None else cap
        return self._top(lambda *a: self._l.sg_window_groups_top_tail(self._h, b, k, min_value, *a), cap, GROUP_EDGE_DTYPE, np.uint32)

    def window_group_nodes_top_tail(self, k: int, min_value: float = float("-inf"), by: str = "in_lat_dev", cap: Optional[int] = None):
        """window_group_nodes_top with the tail rows as the trend source (sg_window_group_nodes_top_tail); by: a key of NSEL_BY."""
        b = self._nby(by)
        return self._top(lambda *a: self._l.sg_window_group_nodes_top_tail(self._h, b, k, min_value, *a),
                         self._node_cap(k, cap, self._l.sg_window_group_nodes), NODE_DTYPE, np.uint32)

    # ---- traffic baselines (K23): each entity's request rate and load against its own past ----
    def set_traffic_trend(self, spaces=("nodes",), params: Optional[dict] = (), **kw):
        """Switch the traffic baselines on (sg_set_traffic_trend): per space ("edges" / "nodes" / "groups" / "group_nodes", or the
        SG_T_* bits as an int; each but "edges" needs its rows on: set_nodes / set_groups / set_group_nodes) a baseline of the
        request count and the busy time of every entity side; TRAFFIC_DEFAULTS' parameters as keywords or a dict, max_entries 0 =
        the default of the mean baseline of each space.  Every call starts empty baselines.  spaces None / 0 or params=None
        switches the stage off."""
        bits = 0 if spaces is None else spaces if isinstance(spaces, int) else self._tbits(spaces)
        self._set_stage("traffic_trend", params, kw, bits)

    @staticmethod
    def _tbits(spaces) -> int:
        bits = 0
        for sp in ([spaces] if isinstance(spaces, str) else spaces):
            if sp not in T_SPACES:
                raise ValueError(f"unknown traffic space {sp!r}: one of {sorted(T_SPACES)}")
            bits |= T_SPACES[sp]
        return bits

    def _tbit(self, space) -> int:
        return space if isinstance(space, int) else self._tbits(space)

    @staticmethod
    def _tby(by, side=None) -> int:
        """SG_TSEL_*: an int as it is; else a direction of TSEL_BY, with side "in" / "out" (TSEL_SIDE) ORed in"""
        if isinstance(by, int):
            return by
        if by not in TSEL_BY or (side is not None and side not in TSEL_SIDE):
            raise ValueError(f"unknown traffic key {by!r} / side {side!r}: one of {sorted(TSEL_BY)}, {sorted(TSEL_SIDE)}")
        return TSEL_BY[by] | (TSEL_SIDE[side] if side is not None else 0)

    def window_traffic(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """TREND_DTYPE traffic rows of the last read window (sg_window_traffic), row k for row k of the window: lat_dev is the RATE
        deviation, err_dev the LOAD deviation, base_mean_us the baseline rate in requests per window; or the rows at `index`."""
        return self._window_rows(self._l.sg_window_traffic, TREND_DTYPE, index)

    def window_node_traffic(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE traffic rows (sg_window_node_traffic), row k for node row k of window_nodes(); or those at `index`."""
        return self._window_rows(self._l.sg_window_node_traffic, NODE_TREND_DTYPE, index)

    def window_group_traffic(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """TREND_DTYPE traffic rows (sg_window_group_traffic), row k for group edge k of window_groups(); or those at `index`."""
        return self._window_rows(self._l.sg_window_group_traffic, TREND_DTYPE, index)

    def window_group_node_traffic(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """NODE_TREND_DTYPE traffic rows (sg_window_group_node_traffic), row k for row k of window_group_nodes(); or those at `index`."""
        return self._window_rows(self._l.sg_window_group_node_traffic, NODE_TREND_DTYPE, index)

    def window_traffic_buffer(self, space) -> int:
        """device pointer of the traffic rows of one space of the window window_run closed last (sg_window_traffic_buffer)"""
        bits = self._tbit(space)
        return self._pointers(lambda h, *a: self._l.sg_window_traffic_buffer(h, bits, *a), 1)[0]

    def traffic_trend_entries(self, space) -> np.ndarray:
        """the traffic baseline of one space in key order, TREND_ENTRY_DTYPE with the keys of the mean baseline of that space;
        lat_mean / lat_dev are 1000 x the request count, err_mean / err_dev the busy time in ns (sg_traffic_trend_entries)"""
        bits = self._tbit(space)
        return self._counted(lambda h, *a: self._l.sg_traffic_trend_entries(h, bits, *a), TREND_ENTRY_DTYPE)

    def traffic_trend_stats(self, space) -> SgTrendStats:
        bits = self._tbit(space)
        return self._stats(lambda h, *a: self._l.sg_traffic_trend_stats_get(h, bits, *a), SgTrendStats)

    def window_nodes_top_traffic(self, k: int, min_value: float = float("-inf"), by="drop", side="in", cap: Optional[int] = None):
        """(the selected node rows, their indices) by a traffic row (sg_window_nodes_top_traffic): by "surge" / "drop" / "load_up" /
        "load_down" of side "in" / "out" (or by as the SG_TSEL_* int), the signed value descending, k = 0 every row >= min_value."""
        b = self._tby(by, side)
        return self._top(lambda *a: self._l.sg_window_nodes_top_traffic(self._h, b, k, min_value, *a), self._node_cap(k, cap), NODE_DTYPE, np.uint32)

    def window_groups_top_traffic(self, k: int, min_value: float = float("-inf"), by="drop", cap: Optional[int] = None):
        """(the selected group edges, their indices) by a traffic row (sg_window_groups_top_traffic); by: a direction of TSEL_BY."""
        b = self._tby(by)
        cap = (k or self.max_edges) if cap is None else cap
        return self._top(lambda *a: self._l.sg_window_groups_top_traffic(self._h, b, k, min_value, *a), cap, GROUP_EDGE_DTYPE, np.uint32)

    def window_group_nodes_top_traffic(self, k: int, min_value: float = float("-inf"), by="drop", side="in", cap: Optional[int] = None):
        """(the selected workload rows, their indices) by a traffic row (sg_window_group_nodes_top_traffic); by, side as
        window_nodes_top_traffic: "the 20 workloads whose inbound traffic fell furthest" is (20, by="drop", side="in")."""
        b = self._tby(by, side)
        return self._top(lambda *a: self._l.sg_window_group_nodes_top_traffic(self._h, b, k, min_value, *a),
                         self._node_cap(k, cap, self._l.sg_window_group_nodes), NODE_DTYPE, np.uint32)

    # ---- SLO burn rates (K24): each service's and workload's error budget over a short and a long span of windows ----
    def set_slo(self, spaces=("group_nodes",), params: Optional[dict] = (), **kw):
        """Switch the SLO stage on (sg_set_slo): per space ("nodes" / "group_nodes", or the SG_Q_* bits as an int; each needs
        set_quantiles on for it) exact sums of requests, errors and slow requests per key and side over the last short_windows and
        long_windows windows, and their burn rates; SLO_DEFAULTS' parameters as keywords or a dict.  Every call starts empty state.
        spaces None / 0 or params=None switches the stage off."""
        bits = 0 if spaces is None else spaces if isinstance(spaces, int) else self._qbits(spaces)
        self._set_stage("slo", params, kw, bits)

    def slo_assign(self, space, refs, objectives) -> None:
        """objective words (slo_objective(); 0 = the defaults) for the keys of refs — KNOWN, LABEL or, in the workload space, GROUP
        refs (sg_slo_assign)"""
        r = np.ascontiguousarray(refs, dtype=np.uint32)
        o = np.ascontiguousarray(objectives, dtype=np.uint32)
        if r.shape != o.shape or r.ndim != 1:
            raise ValueError("refs and objectives are two lists of one length")
        self._ck(self._l.sg_slo_assign(self._h, self._qbit(space), r.ctypes.data, o.ctypes.data, len(r)))

    def window_node_slo(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, SLO_WORDS) u64 SLO rows of the last read window (sg_window_node_slo), row k for row k of window_nodes(); or the rows
        at `index` (only those cross PCIe)"""
        return self._window_rows(self._l.sg_window_node_slo, np.dtype(("<u8", (SLO_WORDS,))), index)

    def window_group_node_slo(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, SLO_WORDS) u64 SLO rows (sg_window_group_node_slo), row k for row k of window_group_nodes(); or those at `index`"""
        return self._window_rows(self._l.sg_window_group_node_slo, np.dtype(("<u8", (SLO_WORDS,))), index)

    def window_slo_buffer(self, space) -> int:
        """device pointer of the SLO rows of one space of the window window_run closed last (sg_window_slo_buffer)"""
        bits = self._qbit(space)
        return self._pointers(lambda h, *a: self._l.sg_window_slo_buffer(h, bits, *a), 1)[0]

    def slo_entries(self, space) -> np.ndarray:
        """(n, SLO_ENTRY_WORDS) u64: the state of one space, a key with traffic in the long span a row, ascending (sg_slo_entries)"""
        bits = self._qbit(space)
        return self._counted(lambda h, *a: self._l.sg_slo_entries(h, bits, *a), np.dtype("<u8"), (SLO_ENTRY_WORDS,))

    def slo_stats(self, space) -> SloStats:
        bits = self._qbit(space)
        return self._stats(lambda h, *a: self._l.sg_slo_stats_get(h, bits, *a), SloStats)

    @staticmethod
    def _sloby(by, side=None) -> int:
        """SG_SLOSEL_*: an int as it is; else a kind of SLOSEL_BY with side "in" / "out" (SLOSEL_SIDE) ORed in"""
        if isinstance(by, int):
            return by
        if by not in SLOSEL_BY or side not in SLOSEL_SIDE:
            raise ValueError(f"unknown SLO key {by!r} / side {side!r}: one of {sorted(SLOSEL_BY)}, {sorted(SLOSEL_SIDE)}")
        return SLOSEL_BY[by] | SLOSEL_SIDE[side]

    def window_nodes_top_slo(self, k: int, min_value_q10: int = 0, by="err", side="in", cap: Optional[int] = None):
        """(the selected node rows, their indices, the row count) by a burn rate (sg_window_nodes_top_slo): by "err" / "slow" of side
        "in" / "out" (or by as the SG_SLOSEL_* int), min(short burn, long burn) descending, k = 0 every row >= min_value_q10."""
        b = self._sloby(by, side)
        return self._top(lambda *a: self._l.sg_window_nodes_top_slo(self._h, b, k, min_value_q10, *a), self._node_cap(k, cap), NODE_DTYPE, np.uint32)

    def window_group_nodes_top_slo(self, k: int, min_value_q10: int = 0, by="err", side="in", cap: Optional[int] = None):
        """(the selected workload rows, their indices, the row count) by a burn rate (sg_window_group_nodes_top_slo): "the 20
        workloads burning their error budget fastest" is (20, 1024, by="err", side="in")."""
        b = self._sloby(by, side)
        return self._top(lambda *a: self._l.sg_window_group_nodes_top_slo(self._h, b, k, min_value_q10, *a),
                         self._node_cap(k, cap, self._l.sg_window_group_nodes), NODE_DTYPE, np.uint32)

    # ---- replica outliers (K25): each pod against the other pods of its workload ----
    def set_replicas(self, params: Optional[dict] = (), **kw):
        """Switch the replica outliers on (sg_set_replicas; needs set_nodes, set_groups and set_group_nodes, and with tail_permille
        set_quantiles over "nodes"): per pod of a workload the error rate, mean latency, load share and tail bin of each side against
        its siblings' leave-one-out remainder.  REPLICA_DEFAULTS' parameters as keywords or a dict (0: the stage's default);
        set_replicas(None) switches it off.  Returns the parameters given."""
        return self._set_stage("replicas", params, kw)

    def window_replicas(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, REPLICA_WORDS) u32 pod rows of the last read window (sg_window_replicas), row k for row k of window_nodes(); or the
        rows at `index`"""
        return self._window_rows(self._l.sg_window_replicas, np.dtype(("<u4", (REPLICA_WORDS,))), index)

    def window_group_replicas(self, index: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, REPLICA_GROUP_WORDS) u32 workload rows (sg_window_group_replicas), row k for row k of window_group_nodes(); or those
        at `index`"""
        return self._window_rows(self._l.sg_window_group_replicas, np.dtype(("<u4", (REPLICA_GROUP_WORDS,))), index)

    def window_replicas_buffer(self) -> tuple:
        """device pointers of the pod rows and the workload rows of the window window_run closed last (sg_window_replicas_buffer)"""
        return self._pointers(self._l.sg_window_replicas_buffer, 2)

    @staticmethod
    def _rselby(by, side=None) -> int:
        """SG_RSEL_*: an int as it is; else a kind of RSEL_BY with side "in" / "out" (RSEL_SIDE) ORed in"""
        if not isinstance(by, str):
            return by
        if by not in RSEL_BY or side not in RSEL_SIDE:
            raise ValueError(f"unknown replica key {by!r} / side {side!r}: one of {sorted(RSEL_BY)}, {sorted(RSEL_SIDE)}")
        return RSEL_BY[by] | RSEL_SIDE[side]

    def window_replicas_top(self, k: int, min_value: int = 0, by="err", side="in", cap: Optional[int] = None):
        """(the selected node rows, their indices, the row count) by a pod row's value (sg_window_replicas_top): by "err" / "lat" /
        "tail" / "share" of side "in" / "out" (or by as the SG_RSEL_* int), descending, k = 0 every judged side with a value >=
        max(min_value, 1).  "The 20 replicas furthest above their peers' error rate" is (20, by="err", side="in")."""
        b = self._rselby(by, side)
        return self._top(lambda *a: self._l.sg_window_replicas_top(self._h, b, k, min_value, *a), self._node_cap(k, cap), NODE_DTYPE, np.uint32)

    @staticmethod
    def _rows_view(ptr, n) -> np.ndarray:
        if n.value == 0:
            z = np.zeros(0, dtype=EDGE_OUT_DTYPE); z.flags.writeable = False
            return z
        buf = (C.c_char * (n.value * EDGE_OUT_DTYPE.itemsize)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=EDGE_OUT_DTYPE)
        a.flags.writeable = False
        return a

    def window_run(self, stream: int = 0): self._ck(self._l.sg_window_run(self._h, stream or None))
    def window_close(self, stream: int = 0): self._ck(self._l.sg_window_close(self._h, stream or None))
    def window_features(self, stream: int = 0): self._ck(self._l.sg_window_features(self._h, stream or None))
    def window_layer(self, l: int, stream: int = 0): self._ck(self._l.sg_window_layer(self._h, l, stream or None))
    def window_score(self, stream: int = 0): self._ck(self._l.sg_window_score(self._h, stream or None))

    def window_score_reset(self, stream: int = 0): self._ck(self._l.sg_window_score_reset(self._h, stream or None))

    def window_run_sharded(self, comm: "RcclComm", stream: int = 0):
        """K1 pass B .. K5 of this shard's window with every exchange, ONE C call (sg_window_run_sharded); rows stay on the device."""
        self._ck(self._l.sg_window_run_sharded(self._h, comm.ptr, stream or None))
    def window_reset(self, stream: int = 0): self._ck(self._l.sg_window_reset(self._h, stream or None))

    def halo_counts(self, world: int) -> np.ndarray:
        out = np.zeros(world, dtype=np.uint32)
        self._ck(self._l.sg_window_halo_counts(self._h, out.ctypes.data, world))
        return out

    def window_close_sharded(self, d_union_ips: int, d_union_n: int, stream: int = 0):
        self._ck(self._l.sg_window_close_sharded(self._h, d_union_ips, d_union_n, stream or None))

    def window_obip_list(self, d_list: int, cap: int, d_n: int, stream: int = 0):
        self._ck(self._l.sg_window_obip_list(self._h, d_list, cap, d_n, stream or None))

    def bind_buffers(self, stats_sum: int, stats_max: int, feat_rows):
        arr = (C.c_void_p * max(1, len(feat_rows)))(*feat_rows)
        self._ck(self._l.sg_bind_buffers(self._h, stats_sum, stats_max, arr, len(feat_rows)))

    def window_read(self, cap: Optional[int] = None) -> np.ndarray:
        return self._capped(lambda out, c, n: self._l.sg_window_read(self._h, out, c, n), cap)

    def window_buffers(self):
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._ck(self._l.sg_window_buffers(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return a.value, b.value, c.value, n.value

    def feat_buffer(self, l: int):
        p, w = C.c_void_p(), C.c_size_t()
        self._ck(self._l.sg_window_feat_buffer(self._h, l, C.byref(p), C.byref(w)))
        return p.value, w.value

    def rows_buffer(self) -> int:
        return self._pointers(self._l.sg_window_rows_buffer, 1)[0]

    def halo_build(self, d_ids: int, cap: int, d_counts: int, stream: int = 0): self._ck(self._l.sg_halo_build(self._h, d_ids, cap, d_counts, stream or None))
    def halo_pack(self, l: int, d_ids: int, n: int, d_rows: int, stream: int = 0): self._ck(self._l.sg_halo_pack(self._h, l, d_ids, n, d_rows, stream or None))
    def halo_unpack(self, l: int, d_ids: int, n: int, d_rows: int, stream: int = 0): self._ck(self._l.sg_halo_unpack(self._h, l, d_ids, n, d_rows, stream or None))

    def window_close_gathered(self, d_gathered: int, stride: int, world: int, stream: int = 0):
        self._ck(self._l.sg_window_close_gathered(self._h, d_gathered, stride, world, stream or None))

    def halo_build_padded(self, d_req: int, capp: int, stream: int = 0): self._ck(self._l.sg_halo_build_padded(self._h, d_req, capp, stream or None))
    def halo_pack_padded(self, l: int, d_serve: int, capp: int, d_rows: int, stream: int = 0): self._ck(self._l.sg_halo_pack_padded(self._h, l, d_serve, capp, d_rows, stream or None))
    def halo_unpack_padded(self, l: int, d_req: int, capp: int, d_rows: int, stream: int = 0): self._ck(self._l.sg_halo_unpack_padded(self._h, l, d_req, capp, d_rows, stream or None))

    def outbound_ips(self) -> np.ndarray:
        return self._counted(self._l.sg_window_outbound_ips, np.uint32)

    def window_hist(self) -> np.ndarray:
        """[rows][16] u32 latency histogram bins of the last read window (engine created with edge_histogram=True)."""
        return self._counted(self._l.sg_window_hist, np.uint32, (16,))

    def stats(self) -> SgStats:
        return self._stats(self._l.sg_stats_get, SgStats)

    def timing_enable(self, mask: int = 1): self._ck(self._l.sg_timing_enable(self._h, int(mask)))
    def timing_reset(self): self._ck(self._l.sg_timing_reset(self._h))
    def timing_stride(self, n: int): self._ck(self._l.sg_timing_stride(self._h, int(n)))

    def timing(self, kernel: int) -> Tuple[float, int]:
        us, n = C.c_double(), C.c_uint64()
        self._ck(self._l.sg_timing_get(self._h, kernel, C.byref(us), C.byref(n)))
        return us.value, n.value

    def set_warm(self, on: bool = True):
        """warm windows on / off at run time (off: every window is rebuilt from nothing; the rows are the same either way)"""
        self._ck(self._l.sg_set_warm(self._h, 1 if on else 0))

    def timing_samples(self, kernel: int, cap: int = 4096) -> np.ndarray:
        """every record of a timing group since timing_reset(), microseconds, in launch order"""
        out = np.zeros(cap, dtype=np.float64); n = C.c_size_t()
        self._ck(self._l.sg_timing_samples(self._h, kernel, out.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)))
        return out[: min(cap, n.value)]

    def latency_probe(self, nbytes: int, steps: int, warm: bool = False, loaded: bool = False) -> float:
        """ns per dependent load through `nbytes` of device memory (HBM: far beyond the Infinity Cache, cold; L2: 2 MiB, warm);
        loaded: 65 536 chains in flight at once, one of them timed"""
        ns = C.c_double()
        self._ck(self._l.sg_latency_probe(self._h, int(nbytes), int(steps), (1 if warm else 0) | (2 if loaded else 0), C.byref(ns)))
        return ns.value

    def clock_probe(self, spin_us: int = 200) -> Tuple[float, float]:
        """(MHz under an all-CU spin launched now, MHz averaged over the pass-A launches since the last call)."""
        a, b = C.c_double(), C.c_double()
        self._ck(self._l.sg_clock_probe(self._h, int(spin_us), C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_stamps(self) -> np.ndarray:
        """[kernel 0..3][workgroup][8] phase stamps (100 MHz ticks); zeros unless SG_ABLATE & 0x100."""
        out = np.zeros((4, 4096, 8), dtype=np.uint64)
        self._ck(self._l.sg_debug_stamps(self._h, out.ctypes.data, out.size))
        return out

    def route(self, events: np.ndarray, world: int) -> np.ndarray:
        ev = np.ascontiguousarray(events)
        out = np.zeros(len(ev), dtype=np.uint32)
        self._ck(self._l.sg_route(self._h, ev.ctypes.data, len(ev), world, out.ctypes.data))
        return out
