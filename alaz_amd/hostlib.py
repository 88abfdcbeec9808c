"""ctypes binding of libsgdatastore.so — the C++ host side (DataStore mirror, L7 packer, GraphDS).
Plumbing only; see alaz_amd/csrc/host/."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from .engine import LIB_PATH as ENGINE_LIB, SLO_WORDS, SgConfig
from .replay import EVENT_DTYPE, L7_WIRE_SIZE

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(_HERE, "lib", "libsgdatastore.so")


#: sgh_workload_edge of host_capi.cpp: one group edge in the reference's vocabulary (GraphDS::WorkloadEdges)
WORKLOAD_EDGE_DTYPE = np.dtype([("from_type", "S12"), ("to_type", "S12"), ("from_uid", "S160"), ("to_uid", "S160")]
                               + [(f, "<u8") for f in ("count", "err_count", "sum_ns", "sumsq_us", "max_ns", "score_q32")]
                               + [(f, "<u4") for f in ("edges", "from_nodes", "alive", "worst_row")] + [("score_max", "<f4"), ("pad", "<u4")])


class EdgeRowC(C.Structure):
    _fields_ = [("from_type", C.c_char * 12), ("to_type", C.c_char * 12), ("from_uid", C.c_char * 160), ("to_uid", C.c_char * 160),
                ("count", C.c_uint32), ("err_count", C.c_uint32), ("sum_ns", C.c_uint64), ("max_ns", C.c_uint64), ("sumsq_us", C.c_uint64),
                ("score", C.c_float), ("lat_z", C.c_float), ("err_ratio", C.c_float), ("alive", C.c_uint32),
                ("p50_us", C.c_uint32), ("p99_us", C.c_uint32)]


class SockInfoC(C.Structure):
    _fields_ = [("pid", C.c_uint32), ("fd", C.c_uint64), ("saddr", C.c_uint32), ("sport", C.c_uint16), ("daddr", C.c_uint32), ("dport", C.c_uint16)]


#: sgh_workload_vanished of host_capi.cpp: one vanished workload dependency (GraphDS::WorkloadVanished); a uid is empty unless its
#: key is a workload's (key type 0)
WORKLOAD_VANISHED_DTYPE = np.dtype([("from_key", "<u8"), ("to_key", "<u8"), ("from_uid", "S160"), ("to_uid", "S160")]
                                   + [(f, "<f8") for f in ("lat_mean", "lat_dev", "err_mean", "err_dev")]
                                   + [(f, "<u4") for f in ("n", "last", "row", "pad")])

#: sgh_workload_node of host_capi.cpp: one workload row (GraphDS::WorkloadNodes) — who it is ("workload" with the owner's UID, or
#: pod / service / outbound), then the engine's sg_node_out as engine.NODE_DTYPE has it
def _workload_node_dtype():
    from .engine import NODE_DTYPE
    return np.dtype([("type", "S16"), ("uid", "S160"), ("row", NODE_DTYPE)])


#: sgh_replica_outlier of host_capi.cpp: one selected replica (GraphDS::WorkloadReplicaOutliers) — the pod's UID, its workload's owner
#: UID, its node row and workload row indices, the pod row's flags and the words of the selected side
def _replica_outlier_dtype():
    return np.dtype([("pod", "S160"), ("workload", "S160"), ("node_index", "<u4"), ("workload_index", "<u4"), ("flags", "<u4"),
                     ("err_excess_q20", "<i4"), ("lat_ratio_q10", "<u4"), ("share_q10", "<u4"), ("tail_pod", "<u4"), ("tail_peers", "<u4"),
                     ("replicas", "<u4")])


#: sgh_workload_culprit of host_capi.cpp: one selected workload of the ranking (GraphDS::WorkloadCulprits) — the workload row as
#: _workload_node_dtype has it, then the engine's sg_node_rank as engine.RANK_DTYPE has it
def _workload_culprit_dtype():
    from .engine import RANK_DTYPE
    return np.dtype([("node", _workload_node_dtype()), ("rank", RANK_DTYPE)])


_lib = None


class H2OutC(C.Structure):
    _fields_ = [("method", C.c_char * 64), ("path", C.c_char * 1100), ("authority", C.c_char * 160), ("protocol", C.c_char * 8),
                ("status_code", C.c_uint32), ("latency", C.c_uint64)]

    def as_tuple(self):
        return (self.method, self.path, self.authority, self.protocol, self.status_code, self.latency)


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("SG_HOST_LIB_PATH") or HOST_LIB       # override: sanitizer builds (tools/asan_host_tests.sh)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `python -m alaz_amd.build`")
        lib = C.CDLL(path)
        P, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
        sig = {
            "sgh_packer_create": (P, []), "sgh_packer_destroy": (None, [P]), "sgh_packer_known_ip": (None, [P, u32, C.c_int]),
            "sgh_packer_pack_wire": (sz, [P, P, sz, P, P, sz]), "sgh_packer_pack_wire_full": (sz, [P, P, sz, P, P, sz]), "sgh_packer_labels": (sz, [P, C.c_char_p, sz]),
            "sgh_packer_dropped_parse": (u64, [P]),
            "sgh_parse_http": (None, [C.c_char_p, sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz]),
            "sgh_graphds_create": (P, [C.c_char_p, C.POINTER(SgConfig), sz]), "sgh_graphds_destroy": (None, [P]),
            "sgh_graphds_persist_pod": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p]),
            "sgh_graphds_persist_service": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p]),
            "sgh_graphds_ingest_wire": (C.c_int, [P, P, sz, P]),
            "sgh_graphds_persist_request": (C.c_int, [P, C.c_int64, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                                      C.c_char_p, u32, C.c_char_p, C.c_int]),
            "sgh_graphds_flush": (C.c_long, [P, C.c_int64, C.POINTER(EdgeRowC), sz]),
            "sgh_sockline_create": (P, [u32, u64]), "sgh_sockline_destroy": (None, [P]),
            "sgh_sockline_add": (None, [P, u64, C.POINTER(SockInfoC)]), "sgh_sockline_get": (C.c_int, [P, u64, u64, C.POINTER(SockInfoC)]),
            "sgh_sockline_seed": (C.c_int, [P, C.c_char_p, u64]),
            "sgh_proc_inode_of_link": (C.c_int, [C.c_char_p, C.c_char_p, sz]),
            "sgh_proc_parse_tcp_line": (C.c_int, [C.c_char_p, C.POINTER(u32), C.POINTER(C.c_uint16), C.POINTER(u32), C.POINTER(C.c_uint16)]),
            "sgh_graphds_pg_statements": (sz, [P]),
            "sgh_graphds_set_proc_root": (None, [P, C.c_char_p, u64, u64, u64]), "sgh_graphds_seed_stats": (None, [P, C.POINTER(u64)]),
            "sgh_sockline_delete_unused": (None, [P]), "sgh_sockline_len": (sz, [P]),
            "sgh_sockline_at": (C.c_int, [P, sz, C.POINTER(u64), C.POINTER(u64), C.POINTER(SockInfoC)]),
            "sgh_graphds_tcp_wire": (sz, [P, P, sz]), "sgh_graphds_socklines": (sz, [P]), "sgh_graphds_sockline": (P, [P, u32, u64]),
            "sgh_sockline_ref_get": (P, [P]), "sgh_sockline_ref_release": (None, [P]),
            "sgh_graphds_sweep": (sz, [P, C.c_int64, C.c_int]),
            "sgh_graphds_labels": (sz, [P, C.c_char_p, sz]), "sgh_graphds_dropped_parse": (u64, [P]), "sgh_graphds_engine": (P, [P]),
            "sgh_graphds_proc_exec": (None, [P, u32]), "sgh_graphds_proc_exit": (None, [P, u32]), "sgh_graphds_sweep_http2": (None, [P]),
            "sgh_graphds_http2_stats": (None, [P, C.POINTER(u64)]),
            "sgh_hpack_create": (P, [u32]), "sgh_hpack_destroy": (None, [P]),
            "sgh_hpack_write": (C.c_long, [P, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(u32), sz]),
            "sgh_hpack_table_len": (sz, [P]), "sgh_hpack_table_size": (u32, [P]),
            "sgh_hpack_table_at": (sz, [P, sz, C.c_char_p, sz, C.POINTER(u32)]),
            "sgh_huffman_decode": (C.c_long, [C.c_char_p, sz, C.c_char_p, sz]), "sgh_huffman_encode": (C.c_long, [C.c_char_p, sz, C.c_char_p, sz]),
            "sgh_go_atoi_u32": (u32, [C.c_char_p, sz]),
            "sgh_h2_create": (P, []), "sgh_h2_destroy": (None, [P]),
            "sgh_h2_event": (C.c_int, [P, u32, u64, C.c_int, C.c_char_p, u32, u64, C.c_int, C.POINTER(H2OutC)]),
            "sgh_h2_proc_exec": (None, [P, u32]), "sgh_h2_proc_exit": (None, [P, u32]), "sgh_h2_conn_closed": (None, [P, u32, u64]),
            "sgh_h2_sweep": (None, [P]), "sgh_h2_pending": (sz, [P]), "sgh_h2_parsers": (sz, [P]),
            "sgh_packer_proc_exec": (None, [P, u32]), "sgh_packer_proc_exit": (None, [P, u32]), "sgh_packer_conn_closed": (None, [P, u32, u64]), "sgh_packer_pg_statements": (sz, [P]),
            "sgh_graphds_edges_json": (C.c_long, [P, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz]),
            "sgh_json_string": (sz, [C.c_char_p, sz, C.c_char_p, sz]),
            "sgh_edges_json_from_rows": (C.c_long, [C.POINTER(EdgeRowC), sz, C.c_int64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz]),
            "sgh_packer_kafka_decode": (None, [P, C.c_int]), "sgh_graphds_kafka_decode": (None, [P, C.c_int]),
            "sgh_kafka_decode": (C.c_long, [C.c_char_p, sz, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, sz]),
            "sgh_kafka_decompress": (C.c_long, [C.c_int, C.c_char_p, sz, C.c_char_p, sz]),
            "sgh_crc32": (u32, [C.c_int, C.c_char_p, sz]), "sgh_xxh32": (u32, [C.c_char_p, sz, u32]),
            "sgh_graphds_create2": (P, [C.c_char_p, P, sz, C.c_int]), "sgh_graphds_counters": (None, [P, P]),
            "sgh_mock_events": (sz, [P, P, sz]), "sgh_mock_table_ops": (sz, [P, P, sz]), "sgh_mock_label_count": (u32, [P]),
            "sgh_graphds_set_selection": (C.c_int, [P, u32, C.c_float]), "sgh_graphds_clear_selection": (None, [P]), "sgh_graphds_sink_rows": (sz, [P]),
            "sgh_mock_flushes": (None, [P, P, C.POINTER(C.c_float)]),
            "sgh_graphds_persist_pod_owned": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
            "sgh_graphds_persist_replicaset": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p]),
            "sgh_graphds_set_workload_groups": (C.c_int, [P, u32]), "sgh_graphds_workload_edges": (C.c_long, [P, P, sz]),
            "sgh_mock_group_ops": (sz, [P, P, sz]),
            "sgh_graphds_persist_service_named": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
            "sgh_graphds_persist_endpoints": (C.c_int, [P, C.c_char_p, C.c_char_p, C.c_char_p, P, P, sz]),
            "sgh_graphds_set_service_binding": (C.c_int, [P, C.c_int]),
            "sgh_graphds_set_workload_impact": (C.c_int, [P, u32, u32]),
            "sgh_graphds_workload_impact": (C.c_long, [P, P, sz, P, P, sz]), "sgh_mock_k22_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_workload_trend": (C.c_int, [P, u32, u32, u32, C.c_uint64]),
            "sgh_graphds_set_workload_vanished": (C.c_int, [P, u32, u32, u32]),
            "sgh_graphds_workload_trends": (C.c_long, [P, P, sz]),
            "sgh_graphds_workload_top": (C.c_long, [P, u32, u32, C.c_float, P, P, sz]),
            "sgh_graphds_workload_vanished": (C.c_long, [P, P, sz]), "sgh_mock_k15_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_workload_nodes": (C.c_int, [P, C.c_int]),
            "sgh_graphds_set_workload_node_trend": (C.c_int, [P, u32, u32, u32, C.c_uint64]),
            "sgh_graphds_workload_nodes": (C.c_long, [P, P, sz]), "sgh_graphds_workload_node_trends": (C.c_long, [P, P, sz]),
            "sgh_graphds_workload_nodes_top": (C.c_long, [P, u32, u32, C.c_float, P, P, sz]), "sgh_mock_k16_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_workload_rank": (C.c_int, [P, C.c_int, u32, u32, u32, C.c_float]),
            "sgh_graphds_workload_culprits": (C.c_long, [P, u32, C.c_float, P, P, sz]), "sgh_mock_k17_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_workload_incidents": (C.c_int, [P, C.c_int, u32, C.c_float]),
            "sgh_graphds_workload_incidents": (C.c_long, [P, P, sz, P, sz, P]), "sgh_mock_k18_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_workload_tracks": (C.c_int, [P, C.c_int, u32, u32]),
            "sgh_graphds_workload_incident_tracks": (C.c_long, [P, P, sz]), "sgh_graphds_workload_tracks_ended": (C.c_long, [P, P, sz]),
            "sgh_mock_k19_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_quantiles": (C.c_int, [P, u32, P, sz]),
            "sgh_graphds_latency": (C.c_long, [P, C.c_int, P, sz, P, sz, P]), "sgh_mock_k20_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_tail_trend": (C.c_int, [P, u32, u32, C.c_int, u32, u32, u32, C.c_uint64]),
            "sgh_graphds_tail_trends": (C.c_long, [P, C.c_int, P, sz]),
            "sgh_graphds_workload_tail_top": (C.c_long, [P, u32, u32, C.c_float, P, P, sz]), "sgh_mock_k21_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_traffic_trend": (C.c_int, [P, u32, C.c_int, u32, u32, u32, C.c_uint64, u32, C.c_uint64]),
            "sgh_graphds_workload_traffic_top": (C.c_long, [P, u32, u32, C.c_float, P, P, sz]), "sgh_mock_k23_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_slo": (C.c_int, [P, u32, C.c_int, u32, u32, u32, u32, u32, u32, C.c_uint64]),
            "sgh_graphds_set_workload_slo": (C.c_int, [P, C.c_char_p, u32]), "sgh_graphds_workload_slo": (C.c_long, [P, P, sz]),
            "sgh_graphds_workload_slo_top": (C.c_long, [P, u32, u32, u32, P, P, sz]), "sgh_mock_k24_ops": (sz, [P, P, sz]),
            "sgh_graphds_set_replica_outliers": (C.c_int, [P, C.c_int, u32, C.c_uint64, u32, u32, u32, u32]),
            "sgh_graphds_workload_replica_outliers": (C.c_long, [P, u32, u32, u32, P, sz]), "sgh_mock_k25_ops": (sz, [P, P, sz]),
        }
        for name, (res, args) in sig.items():
            f = getattr(lib, name); f.restype = res; f.argtypes = args
        _lib = lib
    return _lib


def _labels(fn, h) -> List[str]:
    buf = C.create_string_buffer(1 << 16)
    n = fn(h, buf, len(buf))
    return buf.value.decode().split("\n") if n else []


def parse_http(req: bytes):
    m, p, v, h = (C.create_string_buffer(1200) for _ in range(4))
    load().sgh_parse_http(req, len(req), m, p, v, h, 1200)
    return tuple(x.value.decode("latin-1") for x in (m, p, v, h))


def proc_inode_of_link(link: str):
    buf = C.create_string_buffer(32)
    return buf.value.decode() if load().sgh_proc_inode_of_link(link.encode(), buf, 32) == 0 else None


def proc_parse_tcp_line(line: str):
    """-> (local addr u32, local port, remote addr u32, remote port) or None"""
    la, ra, lp, rp = C.c_uint32(), C.c_uint32(), C.c_uint16(), C.c_uint16()
    if load().sgh_proc_parse_tcp_line(line.encode(), C.byref(la), C.byref(lp), C.byref(ra), C.byref(rp)) != 0:
        return None
    return la.value, lp.value, ra.value, rp.value


SL_ERRORS = {1: "sock line is empty", 2: "closed socket on last entry", 3: "no smaller value found", 4: "closed socket"}


class SocketLine:
    """alaz::SocketLine (csrc/host/sockline.hpp); addresses are numeric IPv4."""
    def __init__(self, pid: int = 0, fd: int = 0, _ref=None):
        # _ref: an owning reference handed out by sgh_graphds_sockline (a line of a GraphDS's tracker: it stays alive here after the
        # tracker dropped it at process exit)
        self._l = load(); self._own = _ref is None; self._ref = _ref
        self._p = self._l.sgh_sockline_create(pid, fd) if self._own else self._l.sgh_sockline_ref_get(_ref)

    def __del__(self):
        try:
            if self._own and self._p:
                self._l.sgh_sockline_destroy(self._p); self._p = None
            elif self._ref:
                self._l.sgh_sockline_ref_release(self._ref); self._ref = None; self._p = None
        except Exception:
            pass

    def add(self, ts: int, si):
        """si = (saddr, sport, daddr, dport) or None for a close"""
        if si is None:
            self._l.sgh_sockline_add(self._p, ts, None)
        else:
            c = SockInfoC(0, 0, si[0], si[1], si[2], si[3]); self._l.sgh_sockline_add(self._p, ts, C.byref(c))

    def get(self, ts: int, now_ns: int = 1):
        out = SockInfoC()
        rc = self._l.sgh_sockline_get(self._p, ts, now_ns, C.byref(out))
        return ((out.saddr, out.sport, out.daddr, out.dport), None) if rc == 0 else (None, SL_ERRORS[rc])

    def delete_unused(self): self._l.sgh_sockline_delete_unused(self._p)

    def seed_from_proc(self, proc_root: str, now_kernel_ns: int) -> int:
        """getConnectionInfo against `proc_root` (aggregator/sock_num_line.go:399-429); 0 = seeded"""
        return self._l.sgh_sockline_seed(self._p, proc_root.encode(), now_kernel_ns)

    def __len__(self): return self._l.sgh_sockline_len(self._p)

    def values(self):
        out = []
        for i in range(len(self)):
            ts, lm, si = C.c_uint64(), C.c_uint64(), SockInfoC()
            o = self._l.sgh_sockline_at(self._p, i, C.byref(ts), C.byref(lm), C.byref(si))
            out.append((ts.value, lm.value, (si.saddr, si.sport, si.daddr, si.dport) if o == 1 else None))
        return out


class Hpack:
    """hpack::Decoder (csrc/host/http2.hpp)."""

    def __init__(self, max_table_size: int = 4096):
        self._l = load(); self._d = self._l.sgh_hpack_create(max_table_size)

    def __del__(self):
        try: self._l.sgh_hpack_destroy(self._d)
        except Exception: pass

    def write(self, block: bytes):
        """-> (rc, fields): rc 0 ok / -1 decoding error; fields emitted by this call"""
        cap = 8 * len(block) + 4096; buf = C.create_string_buffer(cap); lens = (C.c_uint32 * 512)()
        r = self._l.sgh_hpack_write(self._d, block, len(block), buf, cap, lens, 256)
        nf = r if r >= 0 else -r - 1
        out = []; off = 0
        for i in range(nf):
            nl, vl = lens[2 * i], lens[2 * i + 1]
            out.append((buf.raw[off:off + nl], buf.raw[off + nl:off + nl + vl])); off += nl + vl
        return (0 if r >= 0 else -1), out

    def table(self):
        out = []
        for i in range(self._l.sgh_hpack_table_len(self._d)):
            buf = C.create_string_buffer(8192); lens = (C.c_uint32 * 2)()
            self._l.sgh_hpack_table_at(self._d, i, buf, 8192, lens)
            out.append((buf.raw[:lens[0]], buf.raw[lens[0]:lens[0] + lens[1]]))
        return out

    def table_size(self) -> int: return self._l.sgh_hpack_table_size(self._d)


def huffman_decode(b: bytes):
    out = C.create_string_buffer(2 * len(b) + 8)
    r = load().sgh_huffman_decode(b, len(b), out, 2 * len(b) + 8)
    return None if r < 0 else out.raw[:r]


def huffman_encode(b: bytes) -> bytes:
    out = C.create_string_buffer(4 * len(b) + 8)
    r = load().sgh_huffman_encode(b, len(b), out, 4 * len(b) + 8)
    return out.raw[:r]


def go_atoi_u32(b: bytes) -> int: return load().sgh_go_atoi_u32(b, len(b))


def edges_json_from_rows(rows, window_end_ms=0, monitoring_id="", idempotency_key="", node_id="", version="", batch=1000) -> List[str]:
    """rows: [(from_type, from_uid, to_type, to_uid, count, err, sum_ns, max_ns, sumsq_us, score, lat_z, err_ratio, alive[, p50_us, p99_us])] with bytes strings"""
    arr = (EdgeRowC * max(1, len(rows)))()
    for a, r in zip(arr, rows):
        a.from_type, a.from_uid, a.to_type, a.to_uid = r[0], r[1], r[2], r[3]
        a.count, a.err_count, a.sum_ns, a.max_ns, a.sumsq_us, a.score, a.lat_z, a.err_ratio, a.alive = r[4:13]
        if len(r) > 14:
            a.p50_us, a.p99_us = r[13], r[14]
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = load().sgh_edges_json_from_rows(arr, len(rows), window_end_ms, monitoring_id.encode(), idempotency_key.encode(), node_id.encode(), version.encode(), batch, buf, cap)
        if n >= 0:
            return buf.value.decode("utf-8").split("\n") if n else []
        cap = -n + 16


def json_string(b: bytes) -> str:
    n = load().sgh_json_string(b, len(b), None, 0); out = C.create_string_buffer(n + 1)
    load().sgh_json_string(b, len(b), out, n + 1)
    return out.value.decode("utf-8")


class Http2Assembler:
    def __init__(self):
        self._l = load(); self._a = self._l.sgh_h2_create()

    def __del__(self):
        try: self._l.sgh_h2_destroy(self._a)
        except Exception: pass

    def event(self, pid, fd, method_id, payload: bytes, write_ns, tls=False):
        out = H2OutC()
        r = self._l.sgh_h2_event(self._a, pid, fd, method_id, payload, len(payload), write_ns, int(tls), C.byref(out))
        return out.as_tuple() if r else None

    def proc_exec(self, pid): self._l.sgh_h2_proc_exec(self._a, pid)
    def proc_exit(self, pid): self._l.sgh_h2_proc_exit(self._a, pid)
    def conn_closed(self, pid, fd): self._l.sgh_h2_conn_closed(self._a, pid, fd)
    def sweep(self): self._l.sgh_h2_sweep(self._a)
    def pending(self): return self._l.sgh_h2_pending(self._a)
    def parsers(self): return self._l.sgh_h2_parsers(self._a)


KAFKA_STATUS = {0: "ok", 1: "insufficient", 2: "error", 3: "panic"}


def kafka_decode(payload: bytes, method_id: int, api_version: int = 0):
    """kafka::DecodePayload -> (status, [(topic, partition, key, value), ...])"""
    import struct
    st = C.c_int(); cap = 1 << 20; buf = C.create_string_buffer(cap)
    n = load().sgh_kafka_decode(payload, len(payload), method_id, api_version, C.byref(st), buf, cap)
    out = []; off = 0; raw = buf.raw
    for _ in range(n):
        tn, part, kn, vn = struct.unpack_from("<IiII", raw, off); off += 16
        out.append((raw[off:off + tn], part, raw[off + tn:off + tn + kn], raw[off + tn + kn:off + tn + kn + vn])); off += tn + kn + vn
    return KAFKA_STATUS[st.value], out


def kafka_decompress(codec: int, data: bytes):
    cap = 1 << 22; out = C.create_string_buffer(cap)
    r = load().sgh_kafka_decompress(codec, data, len(data), out, cap)
    return None if r < 0 else out.raw[:r]


def crc32(data: bytes, castagnoli: bool = False) -> int: return load().sgh_crc32(int(castagnoli), data, len(data))
def xxh32(data: bytes, seed: int = 0) -> int: return load().sgh_xxh32(data, len(data), seed)


class Packer:
    def __init__(self):
        self._l = load(); self._p = self._l.sgh_packer_create()

    def __del__(self):
        try:
            self._l.sgh_packer_destroy(self._p)
        except Exception:
            pass

    def known_ip(self, ip: int, add: bool = True): self._l.sgh_packer_known_ip(self._p, ip, int(add))

    def pack_wire(self, wire: bytes, kafka_msgs: Optional[np.ndarray] = None, full_copy: bool = False) -> np.ndarray:
        n = len(wire) // L7_WIRE_SIZE
        km = None
        if kafka_msgs is not None:
            kafka_msgs = np.ascontiguousarray(kafka_msgs, dtype=np.uint32); km = kafka_msgs.ctypes.data
            cap = int(kafka_msgs.sum()) + n
        else:
            cap = n * 160 if getattr(self, "_kafka", False) else n      # a 1 KiB payload holds < 160 minimal records
        out = np.zeros(max(cap, 1), dtype=EVENT_DTYPE)
        fn = self._l.sgh_packer_pack_wire_full if full_copy else self._l.sgh_packer_pack_wire
        k = fn(self._p, C.cast(C.c_char_p(wire), C.c_void_p), n, km, out.ctypes.data, cap)
        return out[:k]

    @property
    def labels(self): return _labels(self._l.sgh_packer_labels, self._p)
    @property
    def dropped_parse(self): return self._l.sgh_packer_dropped_parse(self._p)

    def kafka_decode(self, on: bool = True): self._kafka = on; self._l.sgh_packer_kafka_decode(self._p, int(on))
    def proc_exec(self, pid): self._l.sgh_packer_proc_exec(self._p, pid)
    def proc_exit(self, pid): self._l.sgh_packer_proc_exit(self._p, pid)
    def conn_closed(self, pid, fd): self._l.sgh_packer_conn_closed(self._p, pid, fd)
    def pg_statements(self) -> int: return self._l.sgh_packer_pg_statements(self._p)


class GraphDS:
    """C++ GraphDS over the real engine (engine_lib = path of libservicegraph.so) or over a recording
    stand-in (engine_lib=None; host-logic tests)."""

    def __init__(self, cfg: SgConfig, engine_lib: Optional[str] = ENGINE_LIB, batch: int = 4096, divert_requests: bool = False):
        self._l = load()
        self._g = self._l.sgh_graphds_create2(engine_lib.encode() if engine_lib else None, C.byref(cfg), batch, int(divert_requests))
        if not self._g:
            raise RuntimeError("GraphDS: engine could not be created (no usable gfx950 device or library missing); no CPU fallback")
        self.max_edges = int(cfg.max_edges)

    def close(self):
        if self._g:
            self._l.sgh_graphds_destroy(self._g); self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def PersistPod(self, uid: str, ip: str, event_type: str = "ADD"): return self._l.sgh_graphds_persist_pod(self._g, event_type.encode(), uid.encode(), ip.encode())
    def PersistService(self, uid: str, ip: str, event_type: str = "ADD"): return self._l.sgh_graphds_persist_service(self._g, event_type.encode(), uid.encode(), ip.encode())

    def apply_ops(self, ops):
        for kind, et, uid, ip in ops:
            (self.PersistPod if kind == "pod" else self.PersistService)(uid, ip, et)

    def ingest_wire(self, wire: bytes, kafka_msgs: Optional[np.ndarray] = None) -> int:
        n = len(wire) // L7_WIRE_SIZE
        km = None
        if kafka_msgs is not None:
            kafka_msgs = np.ascontiguousarray(kafka_msgs, dtype=np.uint32); km = kafka_msgs.ctypes.data
        buf = (C.c_char * len(wire)).from_buffer_copy(wire)
        return self._l.sgh_graphds_ingest_wire(self._g, C.addressof(buf), n, km)

    def PersistRequest(self, r: Sequence) -> int:
        """r: the 16 ReqInfo slots (datastore/backend.go:824-839)."""
        e = lambda s: s.encode("latin-1")
        return self._l.sgh_graphds_persist_request(self._g, r[0], r[1], e(r[2]), e(r[3]), e(r[4]), e(r[6]), e(r[7]), e(r[8]), e(r[10]), r[11], e(r[13]), int(r[15]))

    def FlushWindow(self, window_end_ms: int = 0):
        out = (EdgeRowC * self.max_edges)()
        n = self._l.sgh_graphds_flush(self._g, window_end_ms, out, self.max_edges)
        if n < 0:
            raise RuntimeError(f"FlushWindow rc={n}")
        d = {}
        for i in range(min(n, self.max_edges)):
            r = out[i]
            d[(r.from_type.decode(), r.from_uid.decode(), r.to_type.decode(), r.to_uid.decode())] = (
                r.count, r.err_count, r.sum_ns, r.max_ns, r.sumsq_us, r.score, r.lat_z, r.err_ratio, r.alive, r.p50_us, r.p99_us)
        return d

    def FlushWindowRows(self, window_end_ms: int = 0):
        """FlushWindow as (n_edges, [(from_type, from_uid, to_type, to_uid, count, err_count, sum_ns, max_ns, sumsq_us, score, lat_z,
        err_ratio, alive, p50_us, p99_us), ...]) in the order the sink received the rows."""
        out = (EdgeRowC * self.max_edges)()
        n = self._l.sgh_graphds_flush(self._g, window_end_ms, out, self.max_edges)
        if n < 0:
            raise RuntimeError(f"FlushWindow rc={n}")
        rows = []
        for i in range(min(self._l.sgh_graphds_sink_rows(self._g), self.max_edges)):
            r = out[i]
            rows.append((r.from_type.decode(), r.from_uid.decode(), r.to_type.decode(), r.to_uid.decode(), r.count, r.err_count, r.sum_ns,
                         r.max_ns, r.sumsq_us, r.score, r.lat_z, r.err_ratio, r.alive, r.p50_us, r.p99_us))
        return n, rows

    # ---- the workload view (K14) ----
    def PersistPodOwned(self, uid: str, ip: str, owner_id: str = "", event_type: str = "ADD"):
        return self._l.sgh_graphds_persist_pod_owned(self._g, event_type.encode(), uid.encode(), ip.encode(), owner_id.encode())

    def PersistReplicaSet(self, uid: str, owner_id: str = "", event_type: str = "ADD"):
        return self._l.sgh_graphds_persist_replicaset(self._g, event_type.encode(), uid.encode(), owner_id.encode())

    def PersistServiceNamed(self, uid: str, ip: str, name: str, namespace: str = "", event_type: str = "ADD"):
        """PersistService with the Service's name and namespace: what the service binding looks its Endpoints up by"""
        return self._l.sgh_graphds_persist_service_named(self._g, event_type.encode(), uid.encode(), ip.encode(), name.encode(), namespace.encode())

    def PersistEndpoints(self, name: str, namespace: str = "", addresses=(), event_type: str = "ADD"):
        """PersistEndpoints of (namespace, name): addresses = [(type, id), ...], ("Pod", pod UID) for a pod behind the Service"""
        n = len(addresses)
        types = (C.c_char_p * max(n, 1))(*[t.encode() for t, _ in addresses])
        ids = (C.c_char_p * max(n, 1))(*[i.encode() for _, i in addresses])
        return self._l.sgh_graphds_persist_endpoints(self._g, event_type.encode(), name.encode(), namespace.encode(), types, ids, n)

    def set_service_binding(self, on: bool = True) -> int:
        """GraphDS::SetServiceBinding: Services join the workload behind them, on or off (rc; needs set_workload_groups)"""
        return self._l.sgh_graphds_set_service_binding(self._g, 1 if on else 0)

    def set_workload_groups(self, max_groups: int = 0) -> int:
        """GraphDS::SetWorkloadGroups: pods are grouped by their top known owner from now on (rc)"""
        return self._l.sgh_graphds_set_workload_groups(self._g, max_groups)

    def workload_edges(self) -> np.ndarray:
        """GraphDS::WorkloadEdges: the last flushed window's group edges, WORKLOAD_EDGE_DTYPE"""
        n = self._l.sgh_graphds_workload_edges(self._g, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadEdges failed: {n}")
        out = np.zeros(max(n, 1), dtype=WORKLOAD_EDGE_DTYPE)
        self._l.sgh_graphds_workload_edges(self._g, out.ctypes.data, n)
        return out[:n]

    def mock_group_ops(self) -> np.ndarray:
        """the stand-in engine's group calls in order: (node id, group) per sg_group_assign pair, (0xFFFFFFFE, max_groups) per sg_set_groups"""
        n = self._l.sgh_mock_group_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 2), dtype=np.uint32)
        self._l.sgh_mock_group_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload baselines (K15) ----
    def set_workload_trend(self, shift: int = 0, warmup: int = 0, ttl: int = 0, max_entries: int = 0) -> int:
        """GraphDS::SetWorkloadTrend: the per-workload-edge baseline on (a 0 = the parameter's default; rc)"""
        return self._l.sgh_graphds_set_workload_trend(self._g, shift, warmup, ttl, max_entries)

    def set_workload_vanished(self, silent_windows: int = 0, min_seen: int = 0, max_rows: int = 0) -> int:
        """GraphDS::SetWorkloadVanished: the list of vanished workload dependencies on (rc)"""
        return self._l.sgh_graphds_set_workload_vanished(self._g, silent_windows, min_seen, max_rows)

    def _rows(self, what, call, dtype, *lead):
        """call(g, *lead, NULL, 0) for the count, then the rows"""
        n = call(self._g, *lead, None, 0)
        if n < 0:
            raise RuntimeError(f"{what} failed: {n}")
        out = np.zeros(max(n, 1), dtype=dtype)
        call(self._g, *lead, out.ctypes.data, n)
        return out[:n]

    def workload_trends(self) -> np.ndarray:
        """GraphDS::WorkloadTrends: the last flushed window's group trend rows (engine.TREND_DTYPE), row k for edge k of workload_edges()"""
        from .engine import TREND_DTYPE
        return self._rows("WorkloadTrends", self._l.sgh_graphds_workload_trends, TREND_DTYPE)

    def workload_vanished(self) -> np.ndarray:
        """GraphDS::WorkloadVanished: the last flushed window's vanished workload dependencies, WORKLOAD_VANISHED_DTYPE"""
        return self._rows("WorkloadVanished", self._l.sgh_graphds_workload_vanished, WORKLOAD_VANISHED_DTYPE)

    def workload_top(self, by: int, k: int, min_value: float = float("-inf")):
        """GraphDS::WorkloadTop: (the selected group edges as WORKLOAD_EDGE_DTYPE, their indices) — by = SG_SEL_*"""
        n = self._l.sgh_graphds_workload_top(self._g, by, k, min_value, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadTop failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=WORKLOAD_EDGE_DTYPE), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_top(self._g, by, k, min_value, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k15_ops(self) -> np.ndarray:
        """the stand-in engine's K15 calls in order, four u64 each: (1, shift, warmup, ttl) per sg_set_group_trend, (2, silent_windows,
        min_seen, max_rows) per sg_set_group_vanished, (3, by, k, the bits of min_value) per sg_window_groups_top"""
        n = self._l.sgh_mock_k15_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k15_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload rows (K16) ----
    def set_workload_nodes(self, on: bool = True) -> int:
        """GraphDS::SetWorkloadNodes: the per-window workload rows on or off (rc)"""
        return self._l.sgh_graphds_set_workload_nodes(self._g, 1 if on else 0)

    def set_workload_node_trend(self, shift: int = 0, warmup: int = 0, ttl: int = 0, max_entries: int = 0) -> int:
        """GraphDS::SetWorkloadNodeTrend: the per-workload baseline on (a 0 = the parameter's default; rc)"""
        return self._l.sgh_graphds_set_workload_node_trend(self._g, shift, warmup, ttl, max_entries)

    def workload_nodes(self) -> np.ndarray:
        """GraphDS::WorkloadNodes: the last flushed window's workload rows — type, uid and row (engine.NODE_DTYPE)"""
        return self._rows("WorkloadNodes", self._l.sgh_graphds_workload_nodes, _workload_node_dtype())

    def workload_node_trends(self) -> np.ndarray:
        """GraphDS::WorkloadNodeTrends: engine.NODE_TREND_DTYPE, row k for row k of workload_nodes()"""
        from .engine import NODE_TREND_DTYPE
        return self._rows("WorkloadNodeTrends", self._l.sgh_graphds_workload_node_trends, NODE_TREND_DTYPE)

    def workload_nodes_top(self, by: int, k: int, min_value: float = float("-inf")):
        """GraphDS::WorkloadNodesTop: (the selected workload rows as workload_nodes() gives them, their indices) — by = SG_NSEL_*"""
        n = self._l.sgh_graphds_workload_nodes_top(self._g, by, k, min_value, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadNodesTop failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=_workload_node_dtype()), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_nodes_top(self._g, by, k, min_value, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k16_ops(self) -> np.ndarray:
        """the stand-in engine's K16 calls in order, four u64 each: (1, on, 0, 0) per sg_set_group_nodes, (2, shift, warmup, ttl) per
        sg_set_group_node_trend, (3, by, k, the bits of min_value) per sg_window_group_nodes_top"""
        n = self._l.sgh_mock_k16_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k16_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload ranking (K17) ----
    def set_workload_rank(self, on: bool = True, iters: int = 0, damping_q8: int = 0, seed: int = 0, seed_min_score: float = 0.0) -> int:
        """GraphDS::SetWorkloadRank: the per-window workload ranking on (a 0 = the parameter's default) or off (rc)"""
        return self._l.sgh_graphds_set_workload_rank(self._g, 1 if on else 0, iters, damping_q8, seed, seed_min_score)

    def workload_culprits(self, k: int, min_share: float = float("-inf")):
        """GraphDS::WorkloadCulprits: (the selected workloads — node: the row as workload_nodes() gives it, rank: engine.RANK_DTYPE —
        and their indices)"""
        n = self._l.sgh_graphds_workload_culprits(self._g, k, min_share, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadCulprits failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=_workload_culprit_dtype()), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_culprits(self._g, k, min_share, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k17_ops(self) -> np.ndarray:
        """the stand-in engine's K17 calls in order, four u64 each: (1, iters, damping_q8, seed) per sg_set_group_rank (all ones in the
        three for NULL), (2, k, the bits of min_share, cap) per sg_window_group_rank_top"""
        n = self._l.sgh_mock_k17_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k17_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload incidents (K18) ----
    def set_workload_incidents(self, on: bool = True, by: int = 0, min_value: float = 0.0) -> int:
        """GraphDS::SetWorkloadIncidents: the per-window workload incident grouping on (by: engine.SG_SEL_*) or off (rc)"""
        return self._l.sgh_graphds_set_workload_incidents(self._g, 1 if on else 0, by, min_value)

    def workload_incidents(self):
        """GraphDS::WorkloadIncidents: (engine.INCIDENT_DTYPE rows of the last flushed window, the u32 incident of every row of
        workload_nodes())"""
        from .engine import INCIDENT_DTYPE
        nn = C.c_size_t(0)
        n = self._l.sgh_graphds_workload_incidents(self._g, None, 0, None, 0, C.byref(nn))
        if n < 0:
            raise RuntimeError(f"WorkloadIncidents failed: {n}")
        out, ni = np.zeros(max(n, 1), dtype=INCIDENT_DTYPE), np.zeros(max(nn.value, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_incidents(self._g, out.ctypes.data, n, ni.ctypes.data, nn.value, C.byref(nn))
        return out[:n], ni[:nn.value]

    def mock_k18_ops(self) -> np.ndarray:
        """the stand-in engine's K18 calls in order, four u64 each: (1, by, the bits of min_value, reserved) per sg_set_group_incidents
        (all ones in the three for NULL), (2, cap, 0, 0) per sg_window_group_incidents, (3, n_index, cap, 0) per
        sg_window_group_node_incident"""
        n = self._l.sgh_mock_k18_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k18_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload impact (K22) ----
    def set_workload_impact(self, max_incidents: int = 256, max_hops: int = 8) -> int:
        """GraphDS::SetWorkloadImpact: the upstream impact of the workload incidents on, or off with (0, 0) (rc)"""
        return self._l.sgh_graphds_set_workload_impact(self._g, max_incidents, max_hops)

    def workload_impact(self):
        """GraphDS::WorkloadImpact: (engine.INCIDENT_DTYPE rows of the last flushed window, (covered, engine.IMPACT_WORDS) u64 impact
        rows: row i belongs to incident i)"""
        from .engine import IMPACT_WORDS, INCIDENT_DTYPE
        ni = C.c_size_t(0)
        n = self._l.sgh_graphds_workload_impact(self._g, None, 0, C.byref(ni), None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadImpact failed: {n}")
        inc, rows = np.zeros(max(ni.value, 1), dtype=INCIDENT_DTYPE), np.zeros((max(n, 1), IMPACT_WORDS), dtype=np.uint64)
        self._l.sgh_graphds_workload_impact(self._g, inc.ctypes.data, ni.value, C.byref(ni), rows.ctypes.data, n)
        return inc[:ni.value], rows[:n]

    def mock_k22_ops(self) -> np.ndarray:
        """the stand-in engine's K22 calls in order, four u64 each: (1, max_incidents, max_hops, 0) per sg_set_group_impact,
        (2, cap, 0, 0) per sg_window_group_impact"""
        n = self._l.sgh_mock_k22_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k22_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the workload tracks (K19) ----
    def set_workload_tracks(self, on: bool = True, quiet_windows: int = 2, max_tracks: int = 0) -> int:
        """GraphDS::SetWorkloadTracks: the workload incidents followed across windows, on or off (rc)"""
        return self._l.sgh_graphds_set_workload_tracks(self._g, 1 if on else 0, quiet_windows, max_tracks)

    def _track_rows(self, read, dtype, what):
        n = read(self._g, None, 0)
        if n < 0:
            raise RuntimeError(f"{what} failed: {n}")
        out = np.zeros(max(n, 1), dtype=dtype)
        read(self._g, out.ctypes.data, n)
        return out[:n]

    def workload_incident_tracks(self) -> np.ndarray:
        """GraphDS::WorkloadIncidentTracks: engine.TRACK_DTYPE rows of the last flushed window, row i the track of workload_incidents()'
        row i"""
        from .engine import TRACK_DTYPE
        return self._track_rows(self._l.sgh_graphds_workload_incident_tracks, TRACK_DTYPE, "WorkloadIncidentTracks")

    def workload_tracks_ended(self) -> np.ndarray:
        """GraphDS::WorkloadTracksEnded: engine.TRACK_ENTRY_DTYPE entries of the workload tracks that went quiet in the last flushed window"""
        from .engine import TRACK_ENTRY_DTYPE
        return self._track_rows(self._l.sgh_graphds_workload_tracks_ended, TRACK_ENTRY_DTYPE, "WorkloadTracksEnded")

    def mock_k19_ops(self) -> np.ndarray:
        """the stand-in engine's K19 calls in order, four u64 each: (1, quiet_windows, max_tracks, reserved) per sg_set_group_tracks
        (all ones in the three for NULL), (2, cap, 0, 0) per sg_window_group_incident_tracks, (3, cap, 0, 0) per
        sg_window_group_tracks_ended"""
        n = self._l.sgh_mock_k19_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k19_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the latency percentiles (K20) ----
    def set_quantiles(self, spaces: int = 1, permille=(500, 990)) -> int:
        """GraphDS::SetQuantiles: spaces as SG_Q_* bits (engine.Q_SPACES; 0 = off), up to engine.Q_MAX per-mille values (rc)"""
        qm = np.ascontiguousarray(permille, dtype=np.uint32)
        return self._l.sgh_graphds_set_quantiles(self._g, spaces, qm.ctypes.data if len(qm) else None, len(qm))

    def _latency(self, which: int, sides: int, index, what: str) -> np.ndarray:
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        ip, ni = (None, 0) if idx is None else (idx.ctypes.data, len(idx))
        words = C.c_size_t(0)
        n = self._l.sgh_graphds_latency(self._g, which, ip, ni, None, 0, C.byref(words))
        if n < 0:
            raise RuntimeError(f"{what} failed: {n}")
        out = np.zeros(max(words.value, 1), dtype=np.uint32)
        self._l.sgh_graphds_latency(self._g, which, ip, ni, out.ctypes.data, words.value, None)
        out = out[:words.value]
        return out.reshape((n, sides, -1) if sides == 2 else (n, -1)) if n else out.reshape((0, sides, 0) if sides == 2 else (0, 0))

    def node_latency(self, index=None) -> np.ndarray:
        """GraphDS::NodeLatency: (n, 2, n_q) u32 microseconds of the last flushed window's node rows (out side, in side)"""
        return self._latency(0, 2, index, "NodeLatency")

    def workload_edge_latency(self, index=None) -> np.ndarray:
        """GraphDS::WorkloadEdgeLatency: (n, n_q) u32 microseconds of the last flushed window's group edges"""
        return self._latency(1, 1, index, "WorkloadEdgeLatency")

    def workload_latency(self, index=None) -> np.ndarray:
        """GraphDS::WorkloadLatency: (n, 2, n_q) u32 microseconds of the last flushed window's workload rows"""
        return self._latency(2, 2, index, "WorkloadLatency")

    def mock_k20_ops(self) -> np.ndarray:
        """the stand-in engine's K20 calls in order, four u64 each: (1, spaces, n_q, the first four per-mille 16 bits each) per
        sg_set_quantiles, (2 / 3 / 4, n_index or all ones without an index, cap, 0) per sg_window_node_quantiles /
        sg_window_group_quantiles / sg_window_group_node_quantiles"""
        n = self._l.sgh_mock_k20_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k20_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the tail baselines (K21) ----
    def set_tail_trend(self, spaces: int = 1, permille: int = 990, on: bool = True, shift: int = 0, warmup: int = 0, ttl: int = 0,
                       max_entries: int = 0) -> int:
        """GraphDS::SetTailTrend: a baseline of the `permille` quantile per space (SG_Q_* bits; 0 or on=False: off; a parameter 0 =
        its default; rc)"""
        return self._l.sgh_graphds_set_tail_trend(self._g, spaces, permille, 1 if on else 0, shift, warmup, ttl, max_entries)

    def _tail_trends(self, which: int, dtype, what: str) -> np.ndarray:
        return self._rows(what, self._l.sgh_graphds_tail_trends, dtype, which)

    def node_tail_trends(self) -> np.ndarray:
        """GraphDS::NodeTailTrends: engine.NODE_TREND_DTYPE, row k for node row k of the last flushed window"""
        from .engine import NODE_TREND_DTYPE
        return self._tail_trends(0, NODE_TREND_DTYPE, "NodeTailTrends")

    def workload_edge_tail_trends(self) -> np.ndarray:
        """GraphDS::WorkloadEdgeTailTrends: engine.TREND_DTYPE, row k for edge k of workload_edges()"""
        from .engine import TREND_DTYPE
        return self._tail_trends(1, TREND_DTYPE, "WorkloadEdgeTailTrends")

    def workload_tail_trends(self) -> np.ndarray:
        """GraphDS::WorkloadTailTrends: engine.NODE_TREND_DTYPE, row k for row k of workload_nodes()"""
        from .engine import NODE_TREND_DTYPE
        return self._tail_trends(2, NODE_TREND_DTYPE, "WorkloadTailTrends")

    def workload_tail_top(self, by: int, k: int, min_value: float = float("-inf")):
        """GraphDS::WorkloadTailTop: (the selected workload rows as workload_nodes() gives them, their indices) — by = SG_NSEL_*,
        ranked by the tail rows"""
        n = self._l.sgh_graphds_workload_tail_top(self._g, by, k, min_value, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadTailTop failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=_workload_node_dtype()), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_tail_top(self._g, by, k, min_value, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k21_ops(self) -> np.ndarray:
        """the stand-in engine's K21 calls in order, four u64 each: (1, spaces, permille, shift or all ones for NULL) per
        sg_set_quantile_trend, (2 / 3 / 4, cap, 0, 0) per sg_window_node_quantile_trend / sg_window_group_quantile_trend /
        sg_window_group_node_quantile_trend, (5, by, k, the bits of min_value) per sg_window_group_nodes_top_tail"""
        n = self._l.sgh_mock_k21_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k21_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the traffic baselines (K23) ----
    def set_traffic_trend(self, spaces: int = 2, on: bool = True, shift: int = 0, warmup: int = 0, ttl: int = 0, max_entries: int = 0,
                          rate_floor: int = 0, load_floor_ns: int = 0) -> int:
        """GraphDS::SetTrafficTrend: a baseline of the request rate and the load per space (SG_T_* bits; 0 or on=False: off; a
        parameter 0 = its default; rc)"""
        return self._l.sgh_graphds_set_traffic_trend(self._g, spaces, 1 if on else 0, shift, warmup, ttl, max_entries, rate_floor, load_floor_ns)

    def workload_traffic_top(self, by: int, k: int, min_value: float = float("-inf")):
        """GraphDS::WorkloadTrafficTop: (the selected workload rows as workload_nodes() gives them, their indices) — by = a
        direction of SG_TSEL_* ORed with SG_TSEL_IN or SG_TSEL_OUT, ranked by the signed traffic deviation"""
        n = self._l.sgh_graphds_workload_traffic_top(self._g, by, k, min_value, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadTrafficTop failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=_workload_node_dtype()), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_traffic_top(self._g, by, k, min_value, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k23_ops(self) -> np.ndarray:
        """the stand-in engine's K23 calls in order, four u64 each: (1, spaces, shift or all ones for NULL, rate_floor |
        load_floor_ns << 32) per sg_set_traffic_trend, (2, by, k, the bits of min_value) per sg_window_group_nodes_top_traffic"""
        n = self._l.sgh_mock_k23_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k23_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the replica outliers (K25) ----
    def set_replica_outliers(self, on: bool = True, min_replicas: int = 0, min_requests: int = 0, min_err_excess_q20: int = 0,
                             min_lat_ratio_q10: int = 0, tail_permille: int = 0, min_tail_bins: int = 0) -> int:
        """GraphDS::SetReplicaOutliers: each pod against the other pods of its workload (0: the engine's default; on=False: off; rc)"""
        return self._l.sgh_graphds_set_replica_outliers(self._g, 1 if on else 0, min_replicas, min_requests, min_err_excess_q20, min_lat_ratio_q10,
                                                        tail_permille, min_tail_bins)

    def workload_replica_outliers(self, by: int, k: int, min_value: int = 0) -> np.ndarray:
        """GraphDS::WorkloadReplicaOutliers: the selected replicas (_replica_outlier_dtype) — by = SG_RSEL_ERR / _LAT / _TAIL / _SHARE ORed
        with SG_RSEL_IN or SG_RSEL_OUT, ranked by that side's value"""
        n = self._l.sgh_graphds_workload_replica_outliers(self._g, by, k, min_value, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadReplicaOutliers failed: {n}")
        out = np.zeros(max(n, 1), dtype=_replica_outlier_dtype())
        self._l.sgh_graphds_workload_replica_outliers(self._g, by, k, min_value, out.ctypes.data, n)
        return out[:n]

    def mock_k25_ops(self) -> np.ndarray:
        """the stand-in engine's K25 calls in order, four u64 each: (1, min_replicas | tail_permille << 32 or all ones for NULL,
        min_requests, min_err_excess_q20 | min_lat_ratio_q10 << 32) per sg_set_replicas, (2, n_index or all ones, cap, 0) per
        sg_window_replicas, (3, by, k, min_value) per sg_window_replicas_top"""
        n = self._l.sgh_mock_k25_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k25_ops(self._g, out.ctypes.data, n)
        return out[:n]

    # ---- the SLO burn rates (K24) ----
    def set_slo(self, spaces: int = 4, on: bool = True, latency_bin: int = 10, latency_target_ppm: int = 990000, error_target_ppm: int = 999000,
                short_windows: int = 2, long_windows: int = 12, min_burn_q10: int = 14746, min_requests: int = 100) -> int:
        """GraphDS::SetSLO: exact sums and burn rates per space (SG_Q_NODES | SG_Q_GROUP_NODES bits; 0 or on=False: off; rc)"""
        return self._l.sgh_graphds_set_slo(self._g, spaces, 1 if on else 0, latency_bin, latency_target_ppm, error_target_ppm, short_windows,
                                           long_windows, min_burn_q10, min_requests)

    def set_workload_slo(self, workload: str, objective: int) -> int:
        """GraphDS::SetWorkloadSLO: the objective word (engine.slo_objective(); 0 = the defaults) of the workload with this owner UID (rc)"""
        return self._l.sgh_graphds_set_workload_slo(self._g, workload.encode(), objective)

    def workload_slo(self) -> np.ndarray:
        """GraphDS::WorkloadSLO: (n, SLO_WORDS) u64, the SLO row of every row of workload_nodes()"""
        n = self._l.sgh_graphds_workload_slo(self._g, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadSLO failed: {n}")
        out = np.zeros((max(n, 1), SLO_WORDS), dtype=np.uint64)
        self._l.sgh_graphds_workload_slo(self._g, out.ctypes.data, n)
        return out[:n]

    def workload_slo_top(self, by: int, k: int, min_value_q10: int = 0):
        """GraphDS::WorkloadSLOTop: (the selected workload rows as workload_nodes() gives them, their indices) — by = SG_SLOSEL_ERR or
        SG_SLOSEL_SLOW ORed with SG_SLOSEL_IN or SG_SLOSEL_OUT, ranked by min(short burn, long burn)"""
        n = self._l.sgh_graphds_workload_slo_top(self._g, by, k, min_value_q10, None, None, 0)
        if n < 0:
            raise RuntimeError(f"WorkloadSLOTop failed: {n}")
        out, idx = np.zeros(max(n, 1), dtype=_workload_node_dtype()), np.zeros(max(n, 1), dtype=np.uint32)
        self._l.sgh_graphds_workload_slo_top(self._g, by, k, min_value_q10, out.ctypes.data, idx.ctypes.data, n)
        return out[:n], idx[:n]

    def mock_k24_ops(self) -> np.ndarray:
        """the stand-in engine's K24 calls in order, four u64 each: (1, spaces, latency_bin | long_windows << 32 or all ones for NULL,
        min_requests) per sg_set_slo, (2, space, ref, objective) per ref of sg_slo_assign, (3, cap, 0, 0) per
        sg_window_group_node_slo, (4, by, k, min_value_q10) per sg_window_group_nodes_top_slo"""
        n = self._l.sgh_mock_k24_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._l.sgh_mock_k24_ops(self._g, out.ctypes.data, n)
        return out[:n]

    def set_selection(self, k: int, min_score: float = float("-inf")) -> int:
        """GraphDS::SetSelection: from the next FlushWindow on only the selected rows reach the sink (rc, SG_EINVAL for k > 16384)."""
        return self._l.sgh_graphds_set_selection(self._g, k, min_score)

    def clear_selection(self): self._l.sgh_graphds_clear_selection(self._g)

    def mock_flushes(self) -> dict:
        """the stand-in engine's flush calls: plain ones, flush_window_top ones, and the last k / min_score it received"""
        a = (C.c_uint32 * 3)(); f = C.c_float(0)
        self._l.sgh_mock_flushes(self._g, a, C.byref(f))
        return {"flush_window": a[0], "flush_window_top": a[1], "k": a[2], "min_score": f.value}

    # ---- f-2: TCP connect events -> socket lines -> alive connections ----
    def tcp_wire(self, recs: bytes) -> int:
        assert len(recs) % 64 == 0
        buf = (C.c_uint8 * len(recs)).from_buffer_copy(recs)
        return self._l.sgh_graphds_tcp_wire(self._g, C.addressof(buf), len(recs) // 64)

    def sockline_count(self) -> int: return self._l.sgh_graphds_socklines(self._g)

    def sockline(self, pid: int, fd: int):
        p = self._l.sgh_graphds_sockline(self._g, pid, fd)
        return SocketLine(_ref=p) if p else None

    def sweep(self, now_ms: int, send_alive: bool = True) -> int: return self._l.sgh_graphds_sweep(self._g, now_ms, int(send_alive))

    def set_proc_root(self, root, first_kernel_ns: int = 0, first_user_ns: int = 0, now_user_ns: int = 0):
        """NewSocketLine(fetch = true): lines created from now on are seeded from `root`/<pid>/... (None = off)"""
        self._l.sgh_graphds_set_proc_root(self._g, root.encode() if root else None, first_kernel_ns, first_user_ns, now_user_ns)

    def pg_statements(self) -> int: return self._l.sgh_graphds_pg_statements(self._g)

    def seed_stats(self):
        out = (C.c_uint64 * 2)(); self._l.sgh_graphds_seed_stats(self._g, out); return out[0], out[1]

    def edges_json(self, monitoring_id="", idempotency_key="", node_id="", version="", batch=1000) -> List[str]:
        """The rows of the last FlushWindow as "/edges/" payloads (edges_payload.hpp), one JSON document per batch."""
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            n = self._l.sgh_graphds_edges_json(self._g, monitoring_id.encode(), idempotency_key.encode(), node_id.encode(), version.encode(), batch, buf, cap)
            if n >= 0:
                return buf.value.decode("utf-8").split("\n") if n else []
            cap = -n + 16

    def kafka_decode(self, on: bool = True): self._l.sgh_graphds_kafka_decode(self._g, int(on))
    def proc_exec(self, pid: int): self._l.sgh_graphds_proc_exec(self._g, pid)
    def proc_exit(self, pid: int): self._l.sgh_graphds_proc_exit(self._g, pid)
    def sweep_http2(self): self._l.sgh_graphds_sweep_http2(self._g)

    def http2_stats(self):
        out = (C.c_uint64 * 5)(); self._l.sgh_graphds_http2_stats(self._g, out)
        return dict(zip(("pending", "parsers", "dropped_not_live", "dropped_unparsed", "dropped_time"), list(out)))

    @property
    def labels(self): return _labels(self._l.sgh_graphds_labels, self._g)
    @property
    def dropped_parse(self): return self._l.sgh_graphds_dropped_parse(self._g)
    @property
    def engine_handle(self): return self._l.sgh_graphds_engine(self._g)

    # engine settings that are not part of the DataStore surface go straight to the C ABI
    def set_clock(self, first_kernel_ns: int, first_user_ns: int):
        from . import engine
        assert engine.load_library().sg_set_clock(self.engine_handle, first_kernel_ns, first_user_ns) == 0

    def load_weights(self, w: np.ndarray):
        from . import engine
        w = np.ascontiguousarray(w, dtype=np.float32)
        assert engine.load_library().sg_load_weights(self.engine_handle, w.ctypes.data, len(w)) == 0

    def counters(self) -> dict:
        a = (C.c_uint64 * 9)()
        self._l.sgh_graphds_counters(self._g, a)
        return dict(zip(("offered", "batches_dropped", "engine_errors", "live_ids", "inner_requests", "inner_kafka", "inner_alive", "inner_pods", "inner_services"), list(a)))

    def mock_events(self) -> np.ndarray:
        n = self._l.sgh_mock_events(self._g, None, 0)
        out = np.zeros(max(n, 1), dtype=EVENT_DTYPE)
        self._l.sgh_mock_events(self._g, out.ctypes.data, n)
        return out[:n]

    def mock_table_ops(self) -> np.ndarray:
        n = self._l.sgh_mock_table_ops(self._g, None, 0)
        out = np.zeros((max(n, 1), 3), dtype=np.uint32)
        self._l.sgh_mock_table_ops(self._g, out.ctypes.data, n)
        return out[:n]

    @property
    def mock_label_count(self): return self._l.sgh_mock_label_count(self._g)
