"""CPU tests of the C++ host side (alaz_amd/csrc/host): the L7 packer and the GraphDS decorator,
against the oracle's restatement of the same reference code and against a recording engine."""
import numpy as np
import pytest

from alaz_amd import build, engine, hostlib, replay, weights
from oracle import pyoracle
from tests.helpers import _wire

CLOCK = (1_000_000_000, 1_700_000_000_000_000_000)


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_all()


def _cfg(nodes=256, edges=4096):
    return engine.make_config(max_known_nodes=nodes, max_edges=edges)


@pytest.mark.parametrize("req", [b"GET /user HTTP1.1", b"GET /a HTTP/1.1\r\nHost: example.com\r\nX: y\r\n\r\n",
                                 b"POST /x?y=1 HTTP/1.1\nHost: h:8080\n", b"GET / HTTP/1.1\r\nHost:nospace\r\nHost: second\r\n",
                                 b"GET / HTTP/1.1\r\nHost:  two-spaces\r\n", b"BROKEN", b"", b"A B C D\nHost: x y\n"])
def test_parse_http_matches_oracle(req):
    """C++ ParseHttpPayload == the oracle's restatement of aggregator/data.go:508-531."""
    assert hostlib.parse_http(req) == pyoracle.parse_http_payload(req)


def test_packer_reproduces_generator_events_and_label_order():
    """BASELINE config 1 as 1096-byte records through the C++ packer: the packed events are the
    generator's, and labels are interned in first-use order (what the oracle does on the wire path)."""
    topo, ev, labels, _ = replay.make_config(1)
    pk = hostlib.Packer()
    for ip in list(topo.pod_ips) + list(topo.svc_ips):
        pk.known_ip(int(ip))
    got = pk.pack_wire(replay.to_wire(ev, labels))
    assert pk.labels == labels and pk.dropped_parse == 0
    for f in ("saddr", "daddr", "host_label", "status", "protocol", "flags", "duration_ns", "write_time_ns"):
        assert np.array_equal(got[f], ev[f]), f


def test_packer_plus_packed_oracle_equals_wire_oracle_mixed_protocols():
    """Payload-dependent decisions (Host interning, SQL keyword filter, Kafka fan-out, reversal) made by
    the C++ packer lead to the same edges as the oracle's full reference path on the same records."""
    topo = replay.make_topology(60, 400, seed=11)
    ev, labels = replay.make_events(topo, 20_000, seed=12, mixed=True, with_raw_outbound=True, with_reverse=True)
    wire = bytearray(replay.to_wire(ev, labels))
    # corrupt some Postgres payloads so that parsePostgresCommand rejects them (no SQL keyword / too short)
    pg = np.flatnonzero(ev["protocol"] == replay.PROTO_POSTGRES)[:50]
    for j, i in enumerate(pg):
        off = int(i) * replay.L7_WIRE_SIZE
        if j % 2:
            wire[off + 36 + 5: off + 36 + 11] = b"xxxxxx"            # "SELECT" -> garbage
        else:
            wire[off + 1060: off + 1064] = (3).to_bytes(4, "little")   # payload_size 3 < 5
    kafka = np.where(ev["protocol"] == replay.PROTO_KAFKA, 1 + (np.arange(len(ev)) % 3), 1).astype(np.uint32)
    wire = bytes(wire)
    W = weights.make_weights(1)
    o_wire = pyoracle.Oracle(*CLOCK); o_wire.apply_ops(topo.k8s_ops())
    o_wire.l7_wire(wire, kafka)
    o_wire.window_close(W, 1)

    pk = hostlib.Packer()
    for ip in list(topo.pod_ips) + list(topo.svc_ips):
        pk.known_ip(int(ip))
    packed = pk.pack_wire(wire, kafka)
    assert pk.dropped_parse == o_wire.dropped_parse > 0
    o_pk = pyoracle.Oracle(*CLOCK); o_pk.apply_ops(topo.k8s_ops())
    o_pk.packed(packed, pk.labels)
    o_pk.window_close(W, 1)
    assert o_pk.edge_dict() == o_wire.edge_dict()
    assert o_pk.labels == o_wire.labels == pk.labels


def test_graphds_table_maintenance_and_id_interning():
    """PersistPod / PersistService mirror aggregator/persist.go:55-71,114-130 into sg_upsert_* / sg_delete_*
    with arrival-order node ids; pods without IP are ignored (persist.go:37-40)."""
    g = hostlib.GraphDS(_cfg(), engine_lib=None)
    g.PersistPod("p1", "10.0.0.1"); g.PersistService("s1", "10.96.0.1"); g.PersistPod("p2", "10.0.0.2")
    g.PersistPod("p1", "10.0.0.9", "UPDATE"); g.PersistPod("noip", ""); g.PersistPod("p2", "10.0.0.2", "DELETE")
    g.PersistService("s1", "10.96.0.1", "DELETE")
    ip = engine.ip_u32
    assert g.mock_table_ops().tolist() == [[1, ip("10.0.0.1"), 0], [3, ip("10.96.0.1"), 1], [1, ip("10.0.0.2"), 2],
                                           [1, ip("10.0.0.9"), 0], [2, ip("10.0.0.2"), 0], [4, ip("10.96.0.1"), 0]]


def test_graphds_l7_tap_and_datastore_tap_produce_the_same_events():
    """IngestL7 (raw event, packer) and PersistRequest (the DTO the reference aggregator would have
    built, here taken from the oracle's ReqInfo rows) must hand the engine the same packed events,
    including the un-reversal of AMQP DELIVER / Redis PUSHED_EVENT and the shared label ids."""
    o = pyoracle.Oracle(0, 0, log_limit=100)       # clock (0,0): StartTime == write_time_ns / 1e6
    ops = [("pod", "ADD", "p1", "10.0.0.1"), ("pod", "ADD", "p2", "10.0.0.2"), ("svc", "ADD", "s1", "10.96.0.1")]
    o.apply_ops(ops)
    A, B, S, X = 0x0A000001, 0x0A000002, 0x0A600001, 0x08080808
    ms = 1_000_000
    recs = b"".join([
        _wire(A, S, wt=5 * ms), _wire(A, X, wt=6 * ms, payload=b"GET / HTTP/1.1\r\nHost: ext.example\r\n"),
        _wire(A, X, wt=7 * ms, payload=b"GET / HTTP/1.1\r\n"), _wire(A, S, wt=8 * ms, tls=1),
        _wire(A, S, wt=9 * ms, proto=2, method=2, status=1, payload=b""),            # AMQP DELIVER: reversed
        _wire(B, S, wt=10 * ms, proto=5, method=2, status=2, payload=b"x"),           # Redis PUSHED_EVENT: reversed
        _wire(A, B, wt=11 * ms, proto=3, method=2, status=2, payload=b"Q\x00\x00\x00\x0dselect 1"),
    ])
    assert o.l7_wire(recs) == 7
    g1 = hostlib.GraphDS(_cfg(), engine_lib=None, batch=2); g1.apply_ops(ops)
    g1.ingest_wire(recs); g1.FlushWindow()
    g2 = hostlib.GraphDS(_cfg(), engine_lib=None, batch=3); g2.apply_ops(ops)
    for r in o.reqinfos():
        g2.PersistRequest(r)
    g2.FlushWindow()
    e1, e2 = g1.mock_events(), g2.mock_events()
    assert len(e1) == len(e2) == 7
    for f in ("saddr", "daddr", "host_label", "status", "protocol", "flags", "duration_ns"):
        assert np.array_equal(e1[f], e2[f]), f
    assert np.array_equal(e1["write_time_ns"] // ms, e2["write_time_ns"] // ms)
    assert (e1["flags"] & 2).tolist() == [0, 0, 0, 0, 2, 2, 0] and (e1["flags"] & 1).tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert g1.labels == g2.labels == ["ext.example"] and g1.mock_label_count == 1


def _go_runes(b: bytes):
    """utf8.DecodeRune semantics: a valid sequence is one rune, anything else is U+FFFD for ONE byte."""
    i = 0
    while i < len(b):
        for n in (1, 2, 3, 4):
            try:
                ch = b[i:i + n].decode("utf-8")
                if len(ch) == 1:
                    yield ch, True; i += n; break
            except UnicodeDecodeError:
                pass
        else:
            yield "\ufffd", False; i += 1


def _go_json_string(b: bytes) -> str:
    """encoding/json's string encoding with the default HTML escaping: the model the C++ encoder follows."""
    out = ['"']
    for ch, valid in _go_runes(b):
        o = ord(ch)
        if not valid: out.append("\\ufffd")
        elif ch == '"': out.append('\\"')
        elif ch == "\\": out.append("\\\\")
        elif ch == "\n": out.append("\\n")
        elif ch == "\r": out.append("\\r")
        elif ch == "\t": out.append("\\t")
        elif ch in "<>&" or o < 0x20 or o in (0x2028, 0x2029): out.append("\\u%04x" % o)
        else: out.append(ch)
    out.append('"')
    return "".join(out)


@pytest.mark.parametrize("raw", [b"", b"plain-uid-123", b'quote"back\\slash', b"ctl\x00\x01\x1f\x7f\n\r\t", b"<script>&amp;</script>",
                                 "snow☃ line sep  \U0001F600".encode(), b"bad\xff\xfe utf8", b"\xc0\xaf overlong", b"\xed\xa0\x80 surrogate",
                                 b"cut\xe2\x82", b"\xf4\x90\x80\x80 too big", "svc.namespace.svc.cluster.local:8080".encode()])
def test_json_string_escaping_follows_encoding_json(raw):
    import json
    got = hostlib.json_string(raw)
    assert got == _go_json_string(raw)
    assert json.loads(got) == "".join(ch for ch, _ in _go_runes(raw))          # and it is JSON


def test_edges_payload_json_round_trip_and_batching():
    """f-3: the "/edges/" payload (edges_payload.hpp): metadata keys of datastore/payload.go:3-8, 15 positional slots per edge (13, 14 = p50 / p99 in us),
    shortest round-trip floats, batches with distinct idempotency keys, nothing sent for an empty window."""
    import json, struct
    f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
    rows = [(b"pod", b"uid-a", b"service", b"uid-b", 10, 1, 123456789012, 99999999, 2**63 + 5, f32(0.731), f32(-1.25e-7), f32(0.1), 0, 4194, 99999),
            (b"pod", b"uid-a", b"outbound", b"api.example.com", 1, 0, 5, 5, 0, f32(1.0), f32(0.0), f32(0.0), 3),
            (b"pod", b'we"ird<uid>', b"outbound", b"8.8.8.8", 4294967295, 4294967295, 2**64 - 1, 2**64 - 1, 2**64 - 1, f32(3.4e38), f32(1e-45), float("nan"), 4294967295)]
    docs = hostlib.edges_json_from_rows(rows, 1700000000123, "mon-1", "idem", "node-7", "v0.0.0", batch=2)
    assert len(docs) == 2
    p0, p1 = (json.loads(d) for d in docs)
    assert list(p0) == ["metadata", "window_end", "edges"] and list(p0["metadata"]) == ["monitoring_id", "idempotency_key", "node_id", "alaz_version"]
    assert p0["metadata"] == {"monitoring_id": "mon-1", "idempotency_key": "idem-1700000000123-0", "node_id": "node-7", "alaz_version": "v0.0.0"}
    assert p1["metadata"]["idempotency_key"] == "idem-1700000000123-1" and p0["window_end"] == p1["window_end"] == 1700000000123
    got = p0["edges"] + p1["edges"]
    assert len(got) == 3 and all(len(e) == 15 for e in got) and got[0][13:] == [4194, 99999] and got[1][13:] == [0, 0]
    for e, r in zip(got, rows):
        assert e[:4] == [r[0].decode(), r[1].decode(), r[2].decode(), r[3].decode()]
        assert e[4:9] == list(r[4:9]) and e[9] == r[12]                                  # integers exact, incl. > 2^63
        for k, v in ((10, r[9]), (11, r[10]), (12, r[11])):
            assert (e[k] is None and v != v) or f32(e[k]) == v                          # float32 round trip; NaN -> null
    assert '"score"' not in docs[0] and "0.731" in docs[0]                               # positional rows, shortest float text
    assert hostlib.edges_json_from_rows([], 5) == []


def test_packwire_in_place_equals_the_full_copy_path_on_every_protocol():
    """f-1: L7Packer::PackWire reads the perf record in place and copies the payload only for the handlers that look at it;
    it must give the same packed events, labels and drop counts as DecodeWire(full 1 KiB copy) + Pack, record for record —
    on a stream that mixes every protocol, stale payload bytes from the previous record included."""
    from tests import h2_builder as hb, kafka_builder as kb
    from tests.h2_builder import _h2_trace
    topo = replay.make_topology(60, 400, seed=31)
    ev, labels = replay.make_events(topo, 6000, seed=32, mixed=True, with_raw_outbound=True, with_reverse=True)
    base = replay.to_wire(ev, labels)
    h2, pids = _h2_trace(topo, 200, seed=33)
    batch = [kb.record(b"k%d" % j, b"v" * 9, offset_delta=j) for j in range(3)]
    kaf = b"".join(kb.l7_record(1 + (i & 1), (kb.fetch_response if i & 1 else kb.produce_request)([(b"t", [(0, kb.record_batch(batch, codec=i % 5))])]),
                                1000 + i, int(topo.pod_ips[i % 20]), int(topo.svc_ips[i % 5]), api_version=11 if i & 1 else 7) for i in range(200))
    recs = [base[i:i + 1096] for i in range(0, len(base), 1096)] + [h2[i:i + 1096] for i in range(0, len(h2), 1096)] + [kaf[i:i + 1096] for i in range(0, len(kaf), 1096)]
    rng = np.random.default_rng(34); order = rng.permutation(len(recs))
    # keep the per-connection order of the HTTP/2 frames: shuffle only the positions of the blocks, not within the h2 stream
    h2_pos = sorted(i for i in order if len(base) // 1096 <= i < (len(base) + len(h2)) // 1096)
    it = iter(h2_pos); order = [next(it) if len(base) // 1096 <= i < (len(base) + len(h2)) // 1096 else int(i) for i in order]
    wire = b"".join(recs[i] for i in order)
    outs = []
    for full in (False, True):
        pk = hostlib.Packer(); pk.kafka_decode(True)
        for ip in list(topo.pod_ips) + list(topo.svc_ips):
            pk.known_ip(int(ip))
        for p in pids:
            pk.proc_exec(p)
        outs.append((pk.pack_wire(wire, full_copy=full), pk.labels, pk.dropped_parse))
    (a, la, da), (b, lb, db) = outs
    assert len(a) == len(b) > 6000 and a.tobytes() == b.tobytes() and la == lb and da == db
    assert {int(x) for x in np.unique(a["protocol"])} >= {1, 2, 3, 4, 5, 6}


def test_graphds_is_safe_under_concurrent_callers():
    """the data store is called from arbitrary goroutines / OS threads.  Eight threads ingest wire records (ctypes
    releases the GIL), one keeps upserting pods and one flushes windows; nothing may be lost or duplicated."""
    import threading
    topo = replay.make_topology(40, 300, seed=41)
    ev, labels = replay.make_events(topo, 16_000, seed=42, mixed=True)
    kafka = np.where(ev["protocol"] == replay.PROTO_KAFKA, 2, 1).astype(np.uint32)
    wire = replay.to_wire(ev, labels)
    g = hostlib.GraphDS(_cfg(nodes=512), engine_lib=None, batch=64)
    g.apply_ops(topo.k8s_ops())
    single = hostlib.GraphDS(_cfg(nodes=512), engine_lib=None, batch=64); single.apply_ops(topo.k8s_ops())
    single.ingest_wire(wire, kafka); single.FlushWindow()
    want = single.mock_events()
    chunks = [(wire[i * 2000 * 1096:(i + 1) * 2000 * 1096], kafka[i * 2000:(i + 1) * 2000]) for i in range(8)]
    stop = threading.Event(); errs = []
    def feeder(c):
        try:
            for j in range(0, 2000, 250):
                g.ingest_wire(c[0][j * 1096:(j + 250) * 1096], c[1][j:j + 250])
        except Exception as e:           # pragma: no cover
            errs.append(e)
    def churn():
        k = 0
        while not stop.is_set():
            g.PersistPod("churn-%d" % (k % 7), "10.200.0.%d" % (k % 7 + 1), "UPDATE"); k += 1
    def flusher():
        while not stop.is_set():
            g.FlushWindow()
    ts = [threading.Thread(target=feeder, args=(c,)) for c in chunks] + [threading.Thread(target=churn), threading.Thread(target=flusher)]
    for t in ts: t.start()
    for t in ts[:8]: t.join()
    stop.set()
    for t in ts[8:]: t.join()
    g.FlushWindow()
    got = g.mock_events()
    assert not errs and len(got) == len(want)
    # label ids are handed out in first-use order, which depends on the interleaving: compare through the label strings
    def canon(a, labs):
        a = a.copy(); names = sorted(set(labs)); rank = {n: i + 1 for i, n in enumerate(names)}
        a["host_label"] = [rank[labs[int(x) - 1]] if x else 0 for x in a["host_label"]]
        return np.sort(a.view(np.uint8).reshape(len(a), -1).copy().view([("k", "V32")]).ravel())
    assert sorted(g.labels) == sorted(single.labels)
    assert np.array_equal(canon(got, g.labels), canon(want, single.labels))   # the same multiset of packed events, whatever the interleaving


def _rec(proto, method, payload, *, fd=7, pid=99, prep=0, wt=1000, status=1):
    from tests.helpers import _wire
    r = bytearray(_wire(0x0A000001, 0x0A000002, proto=proto, method=method, status=status, payload=payload, wt=wt))
    r[0:8] = fd.to_bytes(8, "little"); r[16:20] = pid.to_bytes(4, "little"); r[1072:1076] = prep.to_bytes(4, "little")
    return bytes(r)


def test_mysql_and_mongo_handlers_match_the_reference_rules():
    """parseMySQLCommand (aggregator/data.go:1431-1472) and parseMongoEvent (:1561-1617): which events are dropped, and (in the
    oracle's rows) which path string the reference would have persisted; the C++ packer must keep / drop the same events."""
    my = lambda cmd, body: (len(body) + 1).to_bytes(3, "little") + b"\x00" + bytes([cmd]) + body
    def mongo(opcode, body, kind=0):
        msg = b"\x00" * 4 + bytes([kind]) + body                      # flags, section kind, section
        return (16 + len(msg)).to_bytes(4, "little") + (1).to_bytes(4, "little") + (0).to_bytes(4, "little") + opcode.to_bytes(4, "little") + msg
    def doc(name, value, type_=2):
        el = bytes([type_]) + name + b"\x00" + (len(value) + 1).to_bytes(4, "little") + value + b"\x00"
        return (4 + len(el) + 1).to_bytes(4, "little") + el + b"\x00"
    cases = [  # (record, expected path or None when dropped)
        (_rec(7, 1, my(3, b"SELECT * FROM users")), "SELECT * FROM users"),                     # TEXT_QUERY with a keyword
        (_rec(7, 1, my(3, b"ping")), None),                                                       # no SQL keyword: dropped
        (_rec(7, 1, b"\x01\x00\x00"), None),                                                      # shorter than the 5-byte header
        (_rec(7, 2, my(22, b"INSERT INTO t VALUES (?)"), prep=5), "INSERT INTO t VALUES (?)"),    # PREPARE_STMT: remembered under pid-fd-5
        (_rec(7, 3, my(23, (5).to_bytes(4, "little") + b"\x00\x01")), "INSERT INTO t VALUES (?)"),  # EXEC_STMT 5 -> the statement
        (_rec(7, 3, my(23, (6).to_bytes(4, "little"))), "EXECUTE 6 *values*"),                    # unknown statement id
        (_rec(7, 3, my(23, (5).to_bytes(4, "little")), fd=8), "EXECUTE 5 *values*"),              # other connection
        (_rec(7, 4, my(25, (5).to_bytes(4, "little"))), "CLOSE STMT 5 "),                         # STMT_CLOSE forgets it
        (_rec(7, 3, my(23, (5).to_bytes(4, "little"))), "EXECUTE 5 *values*"),
        (_rec(8, 0, mongo(2013, doc(b"find", b"myCollection"))), "find myCollection"),            # OP_MSG, body section, first element a string
        (_rec(8, 0, mongo(2012, b"whatever")), "compressed mongo event"),                         # OP_COMPRESSED
        (_rec(8, 0, mongo(2013, doc(b"find", b"x", type_=16))), None),                            # "document element not a string": dropped
        (_rec(8, 0, mongo(2004, doc(b"find", b"x"))), None),                                      # other opcode: "could not parse mongo event"
        (_rec(8, 0, mongo(2013, doc(b"find", b"x"), kind=1)), None),                              # document-sequence section: not parsed
        (_rec(8, 0, b"\x10\x00\x00\x00short"), ""),                                               # slice out of range -> recover() -> persisted, empty path
        (_rec(8, 0, mongo(2013, (400).to_bytes(4, "little") + b"\x02find\x00")), ""),             # document longer than the capture: same
    ]
    wire = b"".join(r for r, _ in cases)
    o = pyoracle.Oracle(0, 0, log_limit=100); o.pod("ADD", "p1", "10.0.0.1"); o.pod("ADD", "p2", "10.0.0.2")
    kept = [want for _, want in cases if want is not None]
    assert o.l7_wire(wire) == len(kept) and o.dropped_parse == len(cases) - len(kept)
    assert [r[14] for r in o.reqinfos()] == kept
    assert [r[10] for r in o.reqinfos()] == ["MYSQL"] * 7 + ["MONGO"] * 4
    for full in (False, True):
        pk = hostlib.Packer()
        ev = pk.pack_wire(wire, full_copy=full)
        assert len(ev) == len(kept) and pk.dropped_parse == len(cases) - len(kept)
        assert ev["write_time_ns"].tolist() == [1000] * len(kept) and ev["protocol"].tolist() == [7] * 7 + [8] * 4
    # keep / drop record by record
    for rec, want in cases[:3] + cases[9:]:
        pk = hostlib.Packer(); assert len(pk.pack_wire(rec)) == (want is not None)


def test_postgres_handler_keep_and_drop_rules():
    """parsePostgresCommand (aggregator/data.go:1474-1556) beyond the Parse/Bind known answers of tests/golden/pg_kat.json: simple
    queries need an SQL keyword, CLOSE_OR_TERMINATE passes its bytes through, unknown extended messages are dropped."""
    q = lambda s: b"Q" + (len(s) + 5).to_bytes(4, "big") + s + b"\x00"
    cases = [
        (_rec(3, 2, q(b"select 1")), "select 1\x00"), (_rec(3, 2, q(b"hello world")), None), (_rec(3, 2, b"Q\x00\x00"), None),
        (_rec(3, 1, b"X\x00\x00\x00\x04"), "X\x00\x00\x00\x04"),                       # CLOSE_OR_TERMINATE: the payload as it is
        (_rec(3, 3, b"D\x00\x00\x00\x06P\x00"), None),                                  # Describe in an extended query: not parsed
        (_rec(3, 3, b"P\x00\x00\x00\x10s9\x00"), "PREPARE s9 AS ..."),                  # Parse cut after the name: two parts, "query too long"
        (_rec(3, 3, b"P\x00\x00\x00\x10s9"), None),                                     # not even the name's terminator: one part
        (_rec(3, 0, b"whatever"), ""),                                                  # method Unknown: falls through with ""
    ]
    wire = b"".join(r for r, _ in cases)
    o = pyoracle.Oracle(0, 0, log_limit=100); o.pod("ADD", "p1", "10.0.0.1"); o.pod("ADD", "p2", "10.0.0.2")
    kept = [w for _, w in cases if w is not None]
    assert o.l7_wire(wire) == len(kept)
    assert [r[14] for r in o.reqinfos()] == [w.split("\x00")[0] if "\x00" in w else w for w in kept]     # rows are C strings in the oracle's log
    pk = hostlib.Packer()
    assert len(pk.pack_wire(wire)) == len(kept) and pk.dropped_parse == o.dropped_parse == len(cases) - len(kept)


def test_known_ip_sets_have_map_semantics_not_reference_counts():
    """ADD + UPDATE + DELETE of one pod must leave its IP unknown again (persist.go:55-71 is a map store / delete, not a
    count): afterwards a request to that address is outbound and its Host header is interned as the label.  The reverse
    case too: DELETE of a pod that was never added must not remove a service that holds the same IP."""
    A, X = 0x0A000001, 0x0A000063
    g = hostlib.GraphDS(_cfg(), engine_lib=None, batch=1)
    g.PersistPod("src", "10.0.0.1")
    g.PersistPod("px", "10.0.0.99", "ADD"); g.PersistPod("px", "10.0.0.99", "UPDATE"); g.PersistPod("px", "10.0.0.99", "DELETE")
    g.ingest_wire(_wire(A, X, payload=b"GET / HTTP/1.1\r\nHost: ext.example\r\n"))
    assert g.labels == ["ext.example"] and int(g.mock_events()[-1]["host_label"]) == 1
    g.PersistService("sx", "10.0.0.99", "ADD")
    g.PersistPod("ghost", "10.0.0.99", "DELETE")                   # a pod nobody added: the service's entry stays
    g.ingest_wire(_wire(A, X, payload=b"GET / HTTP/1.1\r\nHost: other.example\r\n"))
    assert g.labels == ["ext.example"] and int(g.mock_events()[-1]["host_label"]) == 0


def test_node_ids_are_recycled_after_the_window_that_could_name_them():
    """Every rollout brings new pod UIDs; ids of pods whose last IP is gone must come back, or a long-running agent hits
    sg_config.max_known_nodes.  16 ids, 40 generations of 6 pods (old and new generation overlap): no engine error;
    an id is only reused after a FlushWindow (the open window may still name it); a DELETE of an unknown UID creates
    nothing; a genuinely full id space is reported (SG_ENOSPC) and counted."""
    g = hostlib.GraphDS(_cfg(nodes=16), engine_lib=None)
    for gen in range(40):
        for k in range(6):
            assert g.PersistPod(f"pod-{gen}-{k}", f"10.1.{gen % 200}.{k + 1}") == 0
        if gen:
            for k in range(6):
                g.PersistPod(f"pod-{gen - 1}-{k}", f"10.1.{(gen - 1) % 200}.{k + 1}", "DELETE")
        g.PersistPod(f"never-seen-{gen}", "10.9.9.9", "DELETE")
        c = g.counters()
        assert c["engine_errors"] == 0 and c["live_ids"] <= 12, (gen, c)
        g.FlushWindow(gen)
        assert g.counters()["live_ids"] <= 6
    ops = g.mock_table_ops()
    assert ops[ops[:, 0] == 1][:, 2].max() < 16                     # every id handed to the engine is inside its id space
    # without a flush in between nothing is reused: the 3rd new pod does not fit beside 6 live + ... ids
    g2 = hostlib.GraphDS(_cfg(nodes=4), engine_lib=None)
    for k in range(4):
        assert g2.PersistPod(f"a{k}", f"10.2.0.{k + 1}") == 0
    g2.PersistPod("a0", "10.2.0.1", "DELETE")
    assert g2.PersistPod("b0", "10.2.0.9") == engine.SG_ENOSPC and g2.counters()["engine_errors"] == 1
    g2.FlushWindow(1)
    assert g2.PersistPod("b0", "10.2.0.9") == 0                       # a0's id is free now
    # the same UID coming back before the flush keeps its id
    g2.PersistPod("a1", "10.2.0.2", "DELETE"); assert g2.PersistPod("a1", "10.2.0.2") == 0
    assert g2.counters()["engine_errors"] == 1


def test_datastore_tap_is_additive_unless_diverted():
    """PersistRequest / PersistKafkaEvent reach the inner data store by default (f-3 is additive: a backend without an
    /edges/ route keeps its per-request rows); divert_requests=True keeps them in the engine only."""
    row = (5, 1000, "10.0.0.1", "pod", "p1", 40000, "10.96.0.1", "service", "s1", 80, "HTTP", 200, "", "GET", "/", False)
    for divert, want in ((False, 3), (True, 0)):
        g = hostlib.GraphDS(_cfg(), engine_lib=None, divert_requests=divert)
        g.PersistPod("p1", "10.0.0.1"); g.PersistService("s1", "10.96.0.1")
        for _ in range(3):
            assert g.PersistRequest(row) == 0
        c = g.counters()
        assert c["inner_requests"] == want and c["offered"] == 3 and c["inner_pods"] == 1 and c["inner_services"] == 1


def test_process_exit_forgets_the_prepared_statements_of_the_pid():
    """processExit (data.go:363-401) deletes every pgStmts key that starts with the pid — also of connections whose
    close was never seen."""
    from tests.helpers import _wire as w
    pk = hostlib.Packer()
    parse = b"P" + (4 + 3 + 9 + 2).to_bytes(4, "big") + b"s1\x00" + b"SELECT 1\x00" + b"\x00\x00"
    A, S = 0x0A000001, 0x0A600001
    def rec(pid, fd):
        r = bytearray(w(A, S, proto=3, method=3, status=1, payload=parse))   # EXTENDED_QUERY: a Parse message
        r[16:20] = pid.to_bytes(4, "little"); r[0:8] = fd.to_bytes(8, "little")
        return bytes(r)
    pk.pack_wire(rec(12, 5) + rec(12, 6) + rec(120, 5) + rec(7, 5))
    assert pk.pg_statements() == 4
    pk.proc_exit(12)                                                   # HasPrefix("12"): pid 12 and pid 120
    assert pk.pg_statements() == 1


def test_streaming_harness_runs_on_the_recording_engine():
    """tools/c5_stream.py (feeder threads -> C++ GraphDS::IngestWire, a dispatcher closing windows) with the recording
    stand-in and a small cluster: the harness itself must work without a GPU — everything offered is accounted for."""
    import json, os, subprocess, sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "c5_stream.py")
    out = subprocess.run([sys.executable, tool, "--mock", "--pods", "200", "--ring", "4096", "--rate", "1e5", "--windows", "2",
                          "--feeders", "3", "--window-s", "0.25", "--chunk", "256"], capture_output=True, text=True, timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert lines, out.stderr[-1500:]
    r = json.loads(lines[-1])
    assert r["windows"] == 2 and r["host_batches_dropped"] == 0 and r["engine_errors"] == 0 and r["ingest_rc_nonzero"] == 0
    assert 0.8e5 < r["offered_events_per_s"] < 1.3e5 and r["labels"] > 0
