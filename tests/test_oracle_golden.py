"""CPU tests: pin the oracle against the reference's own known-answer vectors and the semantics
read from its source, and cross-check the scoring definition with an independent numpy version."""
import json
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from oracle import pyoracle, score_np

from tests.helpers import _wire

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CLOCK = (1_000_000_000, 1_700_000_000_000_000_000)


def test_postgres_parse_bind_known_answers():
    """aggregator/pg_test.go:10-92 TestPostgresParseWithKnownStmt, :94-119 ...UnknownStmt."""
    k = json.load(open(os.path.join(GOLD, "pg_kat.json")))
    o = pyoracle.Oracle()
    ks = k["known_stmt"]
    rc, cmd = o.parse_postgres(k["pid"], k["fd"], k["method"], bytes.fromhex(ks["parse_payload"]))
    assert rc == 0 and cmd == ks["parse_expected"]
    rc, cmd = o.parse_postgres(k["pid"], k["fd"], k["method"], bytes.fromhex(ks["bind_payload"]))
    assert rc == 0 and cmd == ks["bind_expected"] == ks["stored_query"]
    o2 = pyoracle.Oracle()
    rc, cmd = o2.parse_postgres(k["pid"], k["fd"], k["method"], bytes.fromhex(k["unknown_stmt"]["bind_payload"]))
    assert rc == 0 and cmd == k["unknown_stmt"]["bind_expected"]


def test_postgres_simple_query_filters():
    """data.go:1477-1498: <5 bytes or no SQL keyword => error => event dropped."""
    o = pyoracle.Oracle()
    assert o.parse_postgres(1, 1, "SIMPLE_QUERY", b"Q\x00\x00")[0] == -1
    assert o.parse_postgres(1, 1, "SIMPLE_QUERY", b"Q\x00\x00\x00\x09hello")[0] == -1
    rc, q = o.parse_postgres(1, 1, "SIMPLE_QUERY", b"Q\x00\x00\x00\x0dselect 1")
    assert rc == 0 and q == "select 1"
    assert o.parse_postgres(1, 1, "EXTENDED_QUERY", b"X\x00\x00\x00\x04abc")[0] == -1


@pytest.mark.parametrize("req,want", [
    (b"GET /user HTTP1.1", ("GET", "/user", "HTTP1.1", "")),                      # main_benchmark_test.go:562
    (b"GET /a HTTP/1.1\r\nHost: example.com\r\nX: y\r\n\r\n", ("GET", "/a", "HTTP/1.1\r", "example.com")),
    (b"POST /x?y=1 HTTP/1.1\nHost: h:8080\n", ("POST", "/x?y=1", "HTTP/1.1", "h:8080")),
    (b"GET / HTTP/1.1\r\nHost:nospace\r\nHost: second\r\n", ("GET", "/", "HTTP/1.1\r", "second")),  # no space: keeps scanning
    (b"GET / HTTP/1.1\r\nHost:  two-spaces\r\n", ("GET", "/", "HTTP/1.1\r", "")),                  # Split gives "" at [1]
    (b"BROKEN", ("", "", "", "")),
    (b"", ("", "", "", "")),
])
def test_parse_http_payload(req, want):
    """aggregator/data.go:508-531 (strings.Split semantics, TrimSuffix "\\r" on the host only)."""
    assert pyoracle.parse_http_payload(req) == want


def test_int_to_ipv4():
    """aggregator/data.go:1751-1758: big-endian dotted quad."""
    assert pyoracle.int_to_ipv4(0x0A000001) == "10.0.0.1"
    assert pyoracle.int_to_ipv4(0xAC10FF02) == "172.16.255.2"
    assert pyoracle.int_to_ipv4(0) == "0.0.0.0"


def test_simulator_trace_known_answer():
    """The reference simulator's event (main_benchmark_test.go:561-617: payload "GET /user HTTP1.1",
    Status 200, Duration 50, WriteTimeNs = t+10) through processHttpEvent -> setFromToV2 ->
    PersistRequest; expected ReqInfo slots derived from data.go:1208-1249 and backend.go:824-839."""
    sim = json.load(open(os.path.join(GOLD, "sim_kat.json")))
    fk, fu = 5_000, 1_700_000_000_123_456_789
    o = pyoracle.Oracle(fk, fu, log_limit=10)
    o.pod("ADD", "pod-uid-1", "10.0.0.1"); o.svc("ADD", "svc-uid-1", "10.96.0.1")
    wt = fk + sim["write_time_offset_ns"]
    n = o.l7_wire(_wire(0x0A000001, 0x0A600001, status=sim["status"], dur=sim["duration"], wt=wt, payload=sim["payload"].encode()))
    assert n == 1
    start = (fu - (fk - wt)) // 1_000_000
    assert o.reqinfos() == [(start, 50, "10.0.0.1", "pod", "pod-uid-1", 40000, "10.96.0.1", "service", "svc-uid-1", 80,
                             "HTTP", 200, "", "GET", "/user", False)]


def test_join_precedence_and_drops():
    """aggregator/data.go:827-870: src must be a pod (else drop); dst service first, then pod, then
    outbound named by Host header, else by raw IP.  "HTTPS" rewrite :1240-1242."""
    o = pyoracle.Oracle(*CLOCK, log_limit=100)
    o.pod("ADD", "p1", "10.0.0.1"); o.pod("ADD", "p2", "10.0.0.2"); o.svc("ADD", "s1", "10.96.0.1")
    o.svc("ADD", "s-shadow", "10.0.0.2")          # same IP registered as pod AND service: service wins
    o.pod("ADD", "no-ip", "")                     # skipped (persist.go:37-40)
    A, B, S, X = 0x0A000001, 0x0A000002, 0x0A600001, 0x08080808
    recs = b"".join([
        _wire(A, S), _wire(A, B), _wire(S, A),                       # svc ; pod-IP shadowed by svc ; src is not a pod -> drop
        _wire(A, X, payload=b"GET / HTTP/1.1\r\nHost: ext.example\r\n"),    # outbound by Host
        _wire(A, X, payload=b"GET / HTTP/1.1\r\n"),                         # outbound by raw IP
        _wire(A, S, tls=1),                                                 # HTTPS
        _wire(0x01010101, S),                                               # unknown src -> drop
    ])
    assert o.l7_wire(recs) == 5 and o.dropped_src == 2
    rows = o.reqinfos()
    assert [(r[3], r[4], r[7], r[8], r[10]) for r in rows] == [
        ("pod", "p1", "service", "s1", "HTTP"), ("pod", "p1", "service", "s-shadow", "HTTP"),
        ("pod", "p1", "outbound", "ext.example", "HTTP"), ("pod", "p1", "outbound", "8.8.8.8", "HTTP"),
        ("pod", "p1", "service", "s1", "HTTPS")]
    assert o.n_known == 4          # p1, p2, s1, s-shadow ("no-ip" never interned)


def test_table_update_delete_semantics():
    """persist.go:55-71: UPDATE assigns (old IP keys stay), DELETE removes the IP key."""
    o = pyoracle.Oracle(*CLOCK, log_limit=100)
    o.pod("ADD", "p1", "10.0.0.1"); o.pod("ADD", "p2", "10.0.0.2")
    o.pod("UPDATE", "p2", "10.0.0.3")              # second IP for p2; 10.0.0.2 still maps to p2
    A = 0x0A000001
    assert o.l7_wire(_wire(A, 0x0A000002) + _wire(A, 0x0A000003)) == 2
    o.pod("DELETE", "p2", "10.0.0.2")
    assert o.l7_wire(_wire(A, 0x0A000002, payload=b"GET / HTTP/1.1\r\n")) == 1
    assert [(r[7], r[8]) for r in o.reqinfos()] == [("pod", "p2"), ("pod", "p2"), ("outbound", "10.0.0.2")]
    o.pod("DELETE", "p1", "10.0.0.1")
    assert o.l7_wire(_wire(A, 0x0A000003)) == 0 and o.dropped_src == 1


def test_direction_reversal_and_kafka_fanout():
    """AMQP DELIVER / Redis PUSHED_EVENT call ReverseDirection (data.go:1110-1112,1151-1153;
    dto.go:226-231); Kafka persists one event per decoded message (data.go:1043-1076)."""
    o = pyoracle.Oracle(*CLOCK, log_limit=100)
    o.pod("ADD", "p1", "10.0.0.1"); o.svc("ADD", "mq", "10.96.0.9")
    A, S = 0x0A000001, 0x0A600009
    recs = _wire(A, S, proto=2, method=2, status=1, payload=b"") + _wire(A, S, proto=2, method=1, status=1, payload=b"") \
        + _wire(A, S, proto=5, method=2, status=1, payload=b"msg", sport=1111, dport=6379) \
        + _wire(A, S, proto=6, method=1, status=1, payload=b"")
    assert o.l7_wire(recs, kafka_msgs=np.array([1, 1, 1, 3])) == 6
    rows = o.reqinfos()
    assert (rows[0][3], rows[0][4], rows[0][7], rows[0][8], rows[0][13]) == ("service", "mq", "pod", "p1", "DELIVER")
    assert (rows[1][3], rows[1][4], rows[1][7], rows[1][8]) == ("pod", "p1", "service", "mq")
    assert (rows[2][2], rows[2][5], rows[2][6], rows[2][9], rows[2][13]) == ("10.96.0.9", 6379, "10.0.0.1", 1111, "PUSHED_EVENT")
    assert [r[10] for r in rows[3:]] == ["KAFKA"] * 3


def test_start_time_conversion_wraps_like_u64():
    """convertKernelTimeToUserspaceTime (data.go:1740-1743): FirstUser - (FirstKernel - write), in u64."""
    fk, fu = 10_000_000_000, 1_700_000_000_000_000_000
    o = pyoracle.Oracle(fk, fu, log_limit=4)
    o.pod("ADD", "p", "10.0.0.1"); o.svc("ADD", "s", "10.96.0.1")
    o.l7_wire(_wire(0x0A000001, 0x0A600001, wt=fk + 2_500_000) + _wire(0x0A000001, 0x0A600001, wt=fk - 1_000_000))
    assert [r[0] for r in o.reqinfos()] == [(fu + 2_500_000) // 10**6, (fu - 1_000_000) // 10**6]


def test_wire_and_packed_paths_agree_config1():
    """BASELINE config 1 (10k HTTP events / 50 pods / 200 edges): the full 1096-byte path and the
    packed-event path of the oracle give identical edges, and the label interning order matches
    the generator's (= the host packer's)."""
    topo, ev, labels, L = replay.make_config(1)
    W = weights.make_weights(L)
    res = []
    for mode in ("wire", "packed"):
        o = pyoracle.Oracle(*CLOCK)
        o.apply_ops(topo.k8s_ops())
        n = o.l7_wire(replay.to_wire(ev, labels)) if mode == "wire" else o.packed(ev, labels)
        assert n == len(ev) - o.dropped_src and o.dropped_src > 0
        if mode == "wire":
            assert o.labels == labels
        o.window_close(W, L)
        res.append(o.edge_dict())
    assert res[0] == res[1] and len(res[0]) > 200


def test_aggregates_match_numpy_groupby():
    """Integer accumulators of the oracle == an independent numpy group-by over the packed events."""
    topo, ev, labels, L = replay.make_config(1)
    o = pyoracle.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    o.packed(ev, labels)
    o.window_close(weights.make_weights(L), L)
    rows = o.edge_rows()
    known = np.isin(ev["saddr"], topo.pod_ips)
    e = ev[known]
    key = (e["saddr"].astype(np.uint64) << np.uint64(32)) | e["daddr"].astype(np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    assert len(uk) == len(rows)
    cnt = np.bincount(inv); s = np.bincount(inv, weights=e["duration_ns"].astype(np.float64))
    assert sorted(cnt.tolist()) == sorted(rows["count"].tolist())
    assert int(rows["sum_ns"].sum()) == int(e["duration_ns"].astype(np.uint64).sum()) == int(s.sum())
    assert int(rows["err_count"].sum()) == int((e["status"] >= 500).sum())
    us = e["duration_ns"] // np.uint64(1000)
    assert int(rows["sumsq_us"].sum()) == int((us * us).sum())
    assert int(rows["max_ns"].max()) == int(e["duration_ns"].max())


@pytest.mark.parametrize("layers", [1, 2])
def test_scoring_matches_independent_numpy(layers):
    """Part 2 of the oracle (features, SAGE layers, score head) against oracle/score_np.py."""
    topo = replay.make_topology(120, 900, seed=77)
    ev, labels = replay.make_events(topo, 40_000, seed=78, with_raw_outbound=True, with_reverse=True)
    W = weights.make_weights(layers)
    o = pyoracle.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    o.packed(ev, labels)
    o.window_close(W, layers)
    rows = o.edge_rows()
    N, NK, NL = o.n_nodes, o.n_known, len(o.labels)

    def dense(ref):
        t, v = ref >> 30, ref & 0x3FFFFFFF
        return np.where(t == 0, v, np.where(t == 1, NK + v, NK + NL + v))
    frm, to = dense(rows["from_ref"].astype(np.int64)), dense(rows["to_ref"].astype(np.int64))
    kind = np.zeros(N, dtype=np.int64); kind[:topo.n_pods] = 1; kind[topo.n_pods:NK] = 2
    s, z, er, x, h = score_np.score(N, kind, frm, to, rows["count"], rows["err_count"], rows["sum_ns"], rows["max_ns"], rows["sumsq_us"], W, layers)
    assert np.allclose(o.node_features(), x, rtol=0, atol=2e-6)
    assert np.allclose(o.layer_output(layers), h, rtol=1e-5, atol=1e-5)
    assert np.abs(rows["score"] - s).max() < 1e-5
    assert np.allclose(rows["lat_z"], z, rtol=1e-5, atol=1e-5) and np.array_equal(rows["err_ratio"], er)
    assert (rows["score"] > 0).all() and (rows["score"] < 1).all()
    # canonical order: rows sorted by (dense from, dense to), no duplicates
    k = frm * (N + 1) + to
    assert (np.diff(k) > 0).all()


def test_window_reset_and_time_bounds():
    topo, ev, labels, L = replay.make_config(1)
    W = weights.make_weights(L)
    o = pyoracle.Oracle(*CLOCK)
    o.apply_ops(topo.k8s_ops())
    o.packed(ev[:5000], labels); o.window_close(W, L); a = o.edge_dict(); ta = (o.window_tmin, o.window_tmax, o.window_events)
    o.packed(ev[5000:], labels); o.window_close(W, L); b = o.edge_dict()
    o2 = pyoracle.Oracle(*CLOCK); o2.apply_ops(topo.k8s_ops()); o2.packed(ev[5000:], labels); o2.window_close(W, L)
    c = o2.edge_dict()
    # integers identical; scores only to rounding: the label id range is cumulative across windows,
    # so the second window of `o` numbers its nodes differently from a fresh oracle
    assert set(b) == set(c) and a != b
    assert all(b[k][:5] == c[k][:5] and abs(b[k][5] - c[k][5]) < 1e-6 for k in b)
    acc = ev[:5000][np.isin(ev[:5000]["saddr"], topo.pod_ips)]
    assert ta[2] == len(acc)
    conv = lambda w: (CLOCK[1] - (CLOCK[0] - int(w))) // 10**6
    assert ta[0] == conv(acc["write_time_ns"].min()) and ta[1] == conv(acc["write_time_ns"].max())
    assert o.window_close(W, L) == 0          # empty window


def test_generator_is_deterministic_and_splitmix_known_answer():
    # splitmix64 reference outputs for seed 1234567 (Vigna's test vector)
    base = 1234567
    z = replay.splitmix64(base - 0x632BE59BD9B4E019 & 0xFFFFFFFFFFFFFFFF, 3, 0)
    assert [int(v) for v in z] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    a = replay.make_config(1); b = replay.make_config(1)
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert int(replay.hash32(np.array([1], dtype=np.uint32))[0]) == pyoracle.lib().or_hash32(1)


def test_latency_histogram_bins_and_percentiles_known_answers(oracle_lib):
    """f-3 (include/servicegraph.h): bin 0 below 2^17 ns, one bin per octave, bin 15 from 2^31 ns; the q-th percentile is the
    upper edge of the first bin whose cumulative count reaches ceil(count * q / 100), capped at max_ns, in whole microseconds."""
    import ctypes as C
    from alaz_amd import replay
    l = oracle_lib.lib()
    l.or_hist_bin.restype = C.c_uint32; l.or_hist_bin.argtypes = [C.c_uint64]
    l.or_percentile_us.restype = C.c_uint32; l.or_percentile_us.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint32]
    edges = [0, 1, (1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18, 5_000_000, (1 << 31) - 1, 1 << 31, 1 << 40, (1 << 62) - 1]
    want = [0, 0, 0, 1, 1, 2, 6, 14, 15, 15, 15]
    assert [l.or_hist_bin(d) for d in edges] == want
    assert replay.hist_bin(np.array(edges, dtype=np.uint64)).tolist() == want
    rng = np.random.default_rng(1)
    d = rng.integers(1, 1 << 40, 20000, dtype=np.uint64) >> rng.integers(0, 30, 20000).astype(np.uint64)
    assert replay.hist_bin(d).tolist() == [l.or_hist_bin(int(x)) for x in d]

    def pct(h, count, mx, q):
        a = (C.c_uint32 * 16)(*h)
        return l.or_percentile_us(a, count, mx, q)
    h = [0] * 16; h[5] = 98; h[9] = 2                               # 98 requests in [2^21, 2^22) ns, 2 in [2^25, 2^26)
    assert pct(h, 100, 50_000_000, 50) == (1 << 22) // 1000 and pct(h, 100, 50_000_000, 99) == 50_000                    # p99 = bin 9's edge 2^26 = 67.1 ms, capped at max 50 ms
    assert pct(h, 100, 1 << 40, 98) == (1 << 22) // 1000 and pct(h, 100, 1 << 40, 99) == (1 << 26) // 1000
    assert pct([0] * 16, 0, 0, 99) == 0                                                                                     # an edge kept alive only by open connections
    h = [0] * 16; h[15] = 1
    assert pct(h, 1, 3_000_000_000, 50) == 3_000_000                                                                        # open last bin -> max_ns
    h = [1] + [0] * 15
    assert pct(h, 1, 90_000, 50) == 90                                                                                      # capped at max_ns inside bin 0
