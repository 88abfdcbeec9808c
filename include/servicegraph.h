/*
 * servicegraph.h — C ABI of the MI355X-native ServiceGraph engine.
 *
 * This is the drop-in boundary for the hot path of getanteon/alaz:
 *
 *   L7Event -> processL7 -> process<Proto>Event -> setFromToV2 -> ds.PersistRequest
 *   (aggregator/data.go:310-337, 1364-1383, 1208-1249, 827-870; datastore/backend.go:819-847)
 *
 * The reference resolves every L7 event to an edge (FromUID -> ToUID) on the CPU and ships one
 * 16-field row per request.  The engine behind this header does the same resolution on the GPU,
 * accumulates per-edge integer statistics, builds a CSR adjacency, runs GraphSAGE-mean message
 * passing and emits one scored row per *edge* per window.
 *
 * Everything here is plain C: pointers, sizes, fixed-width integers.  All functions return
 * 0 (SG_OK) or a negative SG_E* code and never throw.  They may be called from arbitrary OS
 * threads (cgo hands calls to whichever thread runs the goroutine); calls on one handle are
 * serialised internally.  The library never keeps a caller pointer after the call returns
 * (cgo rule: C must not retain Go memory; datastore/backend.go:824-839 copies out likewise).
 *
 * There is NO CPU fallback.  sg_create() fails with SG_ENODEV when no gfx950 device is usable.
 */
#ifndef SERVICEGRAPH_H
#define SERVICEGRAPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 6u   /* 6: delta windows — sg_stats.windows_delta / windows_plain / last_window_new_edges.  5: warm windows — sg_stats.windows_warm / windows_cold, SG_CFG_NO_WARM, sg_set_warm; sg_timing_samples,
                               sg_latency_probe;
                               4: sg_stats.ingest_waits, sg_geometry.pass_a_teams, sg_clock_probe;
                               3: sg_config begins with its own size (a binding compiled against an older, shorter sg_config is
                               detected instead of read past its end; members added later are zero for it), sg_geometry_get;
                               2: sg_edge_out carries p50_us / p99_us, sg_config.flags, sg_window_hist, sg_flush_window_view */

/* ---- return codes ---------------------------------------------------------------------- */
#define SG_OK        0
#define SG_EINVAL   (-22)  /* bad argument                                                   */
#define SG_ENOMEM   (-12)  /* device or host allocation failed                               */
#define SG_ENODEV   (-19)  /* no usable HIP device / HIP runtime error (see sg_last_error)   */
#define SG_ENOSPC   (-28)  /* a capacity in sg_config was exceeded (edges, outbound ips, …)  */
#define SG_EAGAIN   (-11)  /* staging ring full: the batch was dropped and counted           */
#define SG_ESTATE   (-71)  /* call made in the wrong window phase                            */

/* ---- L7 protocol numbers: the BPF enum, ebpf/l7_req/l7.go:19-29 ------------------------- */
#define SG_PROTO_UNKNOWN  0
#define SG_PROTO_HTTP     1
#define SG_PROTO_AMQP     2
#define SG_PROTO_POSTGRES 3
#define SG_PROTO_HTTP2    4
#define SG_PROTO_REDIS    5
#define SG_PROTO_KAFKA    6
#define SG_PROTO_MYSQL    7
#define SG_PROTO_MONGO    8

/* ---- sg_event.flags -------------------------------------------------------------------- */
#define SG_EV_TLS      0x01u /* L7Event.Tls                          ebpf/l7_req/l7.go:402  */
#define SG_EV_REVERSE  0x02u /* AMQP DELIVER / Redis PUSHED_EVENT: ReverseDirection() after
                                the join            aggregator/data.go:1110-1112,1151-1153  */
#define SG_EV_CONSUME  0x04u /* Kafka CONSUME record (informational) data.go:1043-1076       */
#define SG_EV_ALIVE    0x08u /* not a request: one open TCP connection saddr -> daddr, as
                                sendOpenConnection() reports it  aggregator/data.go:1628-1679.
                                Joined like a request but without a Host header (ToUID of an
                                unknown daddr is the IP, :1671-1672); creates / keeps the edge
                                and adds 1 to its `alive` count; status, duration and
                                write_time_ns are ignored and no request is counted.           */

/*
 * One L7 request, packed.  32 bytes, little-endian, naturally aligned.
 * It carries exactly the fields of l7_req.L7Event (ebpf/l7_req/l7.go:396-417) that decide the
 * edge identity and the per-edge statistics; the 1 KiB payload stays on the host.
 *
 *  saddr/daddr  numeric a<<24|b<<16|c<<8|d, as in L7Event.Saddr/Daddr (l7.go:413,415), i.e. the
 *               value IntToIPv4() formats (aggregator/data.go:1751-1767).
 *  host_label   0, or a host-interned id (>=1) of the HTTP "Host:" header value that
 *               parseHttpPayload extracts (data.go:508-531).  Only consulted when daddr is neither
 *               a service nor a pod IP: ToUID = Host header (data.go:851-854).
 *  status       L7Event.Status (HTTP status code, or the 1/2/3 protocol status of
 *               ebpf/c/{postgres,redis,mysql}.c), saturated to 16 bits.
 *  protocol     SG_PROTO_*.
 *  duration_ns  L7Event.Duration, Request.Latency (data.go:1220).
 *  write_time_ns L7Event.WriteTimeNs (kernel monotonic); StartTime is derived as
 *               convertKernelTimeToUserspaceTime()/1e6 (data.go:1219,1740-1743).
 */
typedef struct sg_event {
    uint32_t saddr;
    uint32_t daddr;
    uint32_t host_label;
    uint16_t status;
    uint8_t  protocol;
    uint8_t  flags;
    uint64_t duration_ns;
    uint64_t write_time_ns;
} sg_event;

/* ---- node references -------------------------------------------------------------------- *
 * A node of the service map is what the reference calls (Type, UID): FromType/FromUID,
 * ToType/ToUID (datastore/dto.go:177-195).  Across this ABI a node is a tagged 32-bit ref:
 *   KNOWN  pod or service; payload = the id the host passed to sg_upsert_pod/_service
 *          (the host interns UID -> id in arrival order).
 *   LABEL  outbound, named by a Host header; payload = host_label - 1.
 *   OBIP   outbound, named by the raw destination IP (data.go:862-863); payload = index into
 *          the window's ascending outbound-IP list (sg_window_outbound_ips).
 */
#define SG_REF_TYPE(r)    ((uint32_t)(r) >> 30)
#define SG_REF_VALUE(r)   ((uint32_t)(r) & 0x3FFFFFFFu)
#define SG_REF_KNOWN      0u
#define SG_REF_LABEL      1u
#define SG_REF_OBIP       2u
#define SG_MAKE_REF(t, v) (((uint32_t)(t) << 30) | ((uint32_t)(v) & 0x3FFFFFFFu))

/* node kinds stored per KNOWN id */
#define SG_NODE_POD       1u
#define SG_NODE_SERVICE   2u

/*
 * One scored edge of a closed window.  Rows come out sorted by (dense(from), dense(to)) where
 * dense() orders KNOWN ids first, then LABEL, then OBIP — the canonical CSR order.
 *
 *  count/err_count/sum_ns/max_ns/sumsq_us  integer accumulators over the window's events on this
 *        edge: bit-exact.  "error" = HTTP/HTTP2 status >= 500, or status == 2 for
 *        POSTGRES/REDIS/MYSQL (ebpf/c/postgres.c:91, redis.c:10, mysql.c:36).
 *        sumsq_us = sum of (duration_ns / 1000)^2, wrapping u64.
 *  score      GraphSAGE + factorised MLP anomaly score in (0,1)          (fp32, |d| <= 1e-5)
 *  lat_z      (mean_us(edge) - mean_us(src out-events)) / max(std_us(src), 1)  (fp32)
 *  err_ratio  err_count / count                                            (fp32)
 *  p50_us / p99_us  latency percentiles from the edge's log2 histogram, 0 unless the engine was created with
 *        SG_CFG_EDGE_HISTOGRAM.  Bin of a duration d (ns): 0 for d < 2^17 (131 us), k = floor(log2 d) - 16 for
 *        2^17 <= d < 2^31, 15 for d >= 2^31 (2.1 s): one bin per octave.  The q-th percentile is reported as the upper
 *        edge of the first bin whose cumulative count reaches ceil(count * q / 100) — 2^(17+k) ns, max_ns for the open
 *        last bin — capped at max_ns, in microseconds (floor); 0 for an edge without requests.  Integer arithmetic
 *        throughout: bit-exact.  The bins themselves: sg_window_hist().
 */
#define SG_HIST_BINS 16u
typedef struct sg_edge_out {
    uint64_t sum_ns;
    uint64_t max_ns;
    uint64_t sumsq_us;
    uint32_t from_ref;
    uint32_t to_ref;
    uint32_t count;
    uint32_t err_count;
    float    score;
    float    lat_z;
    float    err_ratio;
    uint32_t alive;             /* open connections reported on this edge in the window (SG_EV_ALIVE) */
    uint32_t p50_us;
    uint32_t p99_us;
} sg_edge_out;

typedef struct sg_config {
    uint32_t struct_size;       /* sizeof(sg_config) as the CALLER compiled it.  sg_create accepts any size from the ABI-3
                                   layout (88 bytes) up to its own; members beyond the caller's size read as zero         */
    uint32_t abi_version;       /* SG_ABI_VERSION                                              */
    int32_t  device;            /* HIP device ordinal                                          */
    uint32_t max_known_nodes;   /* capacity of the pod+service id space                        */
    uint32_t max_labels;        /* capacity of the Host-header label space                     */
    uint32_t max_outbound_ips;  /* distinct raw-IP outbound destinations per window            */
    uint32_t max_ips;           /* distinct pod+service IPs in the join tables                 */
    uint64_t max_edges;         /* distinct edges per window                                   */
    uint32_t max_batch;         /* largest n accepted by one sg_ingest()                       */
    uint32_t layers;            /* GraphSAGE layers L, 1..SG_MAX_LAYERS                         */
    uint32_t rank;              /* this shard                                                   */
    uint32_t world;             /* number of shards (1 = unsharded)                             */
    uint32_t k1_variant;        /* 0 = auto: partitioned LDS aggregation when the graph fits it — 8-byte records sorted by
                                       partition in LDS before they are written, from max_edges >= 2^18 or max_window_events
                                       > 2^21 up; the 16-byte-record form of 2 for smaller windows, with SG_CFG_EDGE_HISTOGRAM
                                       and for node spaces beyond 2^24,
                                   1 = global edge table + device-scope atomics (any size),
                                   2 = partitioned aggregation with 16-byte records (the round-2 kernels),
                                   3 = as 0, but the 8-byte form whatever the window's size (where the graph fits it)  */
    uint64_t max_window_events; /* most events one window may carry (sizes the K1 record slabs;
                                   0 = max_batch)                                               */
    uint32_t windows_in_flight; /* 1..8 window slots, each with its own buffers and HIP stream:
                                   sg_window_run() closes the current window on its slot's stream
                                   and moves on to the next slot, so the (latency-bound) close of
                                   window w overlaps the ingest of window w+1.  0 = 1.              */
    uint32_t max_alive;         /* most SG_EV_ALIVE records one window may carry (0 = 65536)        */
    uint32_t flags;             /* SG_CFG_*                                                          */
} sg_config;

#define SG_CFG_EDGE_HISTOGRAM 0x1u /* keep a 16-bin log2 latency histogram per edge (p50_us / p99_us in the rows, the bins through
                                      sg_window_hist).  Costs LDS in both K1 passes (smaller edge cache, half-size partitions) and
                                      64 bytes per edge of extra traffic: off by default.                                          */

#define SG_CFG_NO_WARM 0x2u        /* never carry the edge set from one window to the next: every window is rebuilt from nothing (see
                                      sg_set_warm).  By default an engine on the 8-byte-record path without the histogram and with
                                      max_edges >= 2^18 keeps the union of the edges its windows have touched, in CSR order: a
                                      window whose edges are all among the kept ones skips the degree count, the row scan, the
                                      scatter and the row sort.  The rows of a window are the same either way, bit for bit.         */
#define SG_CFG_WARM    0x4u        /* keep that state below 2^18 edges too (where it does not pay: for tests)                       */

#define SG_MAX_LAYERS 4u
#define SG_F_IN    32u   /* node feature width                                                  */
#define SG_F_HID   64u   /* hidden width of every SAGE layer and of the score head               */
#define SG_F_EDGE   8u   /* edge feature width                                                  */
#define SG_NODE_STAT_SUM_WORDS 12u /* u64 words per node in the SUM-reduced stats block           */
#define SG_NODE_STAT_MAX_WORDS  2u /* u64 words per node in the MAX-reduced stats block           */

typedef struct sg_stats {
    uint64_t events_in;            /* events handed to K1 since create                         */
    uint64_t events_dropped_src;   /* saddr not a pod IP (data.go:829-832)                     */
    uint64_t events_dropped_ring;  /* SG_EAGAIN drops                                          */
    uint64_t events_dropped_cap;   /* edge / outbound-ip capacity overflow                     */
    uint64_t windows;              /* closed windows                                           */
    uint64_t last_window_events;   /* accepted events in the last closed window                */
    uint64_t last_window_edges;
    uint64_t last_window_nodes;
    int64_t  last_window_tmin_ms;  /* min/max Request.StartTime in the window (data.go:1219)    */
    int64_t  last_window_tmax_ms;
    uint64_t h2d_bytes;
    uint64_t events_misrouted;     /* world > 1: events fed to the wrong shard (see sg_route)    */
    uint64_t halo_overflow;        /* halo requests beyond the per-pair capacity (must be 0)     */
    uint64_t alive_in;             /* SG_EV_ALIVE records handed to K1 since create               */
    uint64_t alive_dropped;        /* ... of which beyond max_alive, or with an endpoint that was dropped */
    uint64_t join_word_updates;    /* join-table words changed in place on the device (incremental upserts/deletes) */
    uint64_t join_full_uploads;    /* whole join-table images uploaded (first build, rebuilds)        */
    uint64_t ingest_waits;         /* sg_ingest / sg_ingest_pinned calls that found a window boundary being marked (sg_flush_begin) and
                                      waited for it — bounded by the staging copies in flight; the reference's PersistRequest blocks on a
                                      full channel instead (datastore/backend.go:844), this is the only wait on the aggregator's thread */
    uint64_t windows_warm;         /* of the windows READ so far (sg_flush_* / sg_window_read): closed on the warm path ...             */
    uint64_t windows_cold;         /* ... by the full rebuild (always, for an engine that keeps no state: then both stay 0)            */
    uint64_t windows_delta;        /* of windows_warm: windows that met edges the kept set lacked and merged them in (ABI 6)           */
    uint64_t windows_plain;        /* windows of a state-keeping engine closed WITHOUT touching the kept state (the host's back-off after
                                      repeated fall-backs, raw-outbound-IP streams): counted in neither windows_warm nor windows_cold    */
    uint64_t last_window_new_edges;/* edges the last read window added to the kept set                                                  */
} sg_stats;

typedef struct sg_engine* sg_handle;

/* ---- lifecycle -------------------------------------------------------------------------- */
int  sg_create(const sg_config* cfg, sg_handle* out);
int  sg_destroy(sg_handle h);
const char* sg_last_error(sg_handle h);          /* thread-unsafe diagnostic string             */
uint32_t sg_abi_version(void);
size_t   sg_weights_count(uint32_t layers);      /* number of fp32 values sg_load_weights wants  */

/* ---- join tables: replaces ClusterInfo.PodIPToPodUid / ServiceIPToServiceUid ------------- *
 * (aggregator/cluster.go:13-17) and their maintenance in processPod / processSvc
 * (aggregator/persist.go:55-71, 114-130).  ADD and UPDATE are both "upsert"; DELETE erases the
 * IP.  Pods without an IP are skipped by the caller (persist.go:37-40).                        */
int sg_upsert_pod(sg_handle h, uint32_t ip, uint32_t node_id);
int sg_delete_pod(sg_handle h, uint32_t ip);
int sg_upsert_service(sg_handle h, uint32_t ip, uint32_t node_id);
int sg_delete_service(sg_handle h, uint32_t ip);

/* FirstKernelTime / FirstUserspaceTime (ebpf/l7_req/l7.go:707-710) for StartTime conversion.   */
int sg_set_clock(sg_handle h, uint64_t first_kernel_ns, uint64_t first_user_ns);

/* Number of Host-header labels the host packer has interned so far (labels are cumulative).
 * The engine also tracks the largest label id it has seen; the larger of the two sizes the
 * LABEL id range of the next closed window.                                                    */
int sg_set_label_count(sg_handle h, uint32_t n_labels);

/* fp32 weight blob, layout documented in DESIGN.md §"weights"; copied.  A close is scored with
 * the blob that was loaded when the close began: a call made while closes are still queued on
 * the device (sg_flush_begin before sg_flush_end, sg_window_run with windows in flight, the
 * staged sg_window_* calls) first waits for their layer and score kernels, then replaces the
 * blob.  Closes begun after it returns use the new blob.                                      */
int sg_load_weights(sg_handle h, const float* w, size_t n);

/* ---- ingest: replaces processL7 .. setFromToV2 .. PersistRequest for the edge fields ------ *
 * sg_ingest copies n events from host memory into the engine's pinned staging ring, uploads
 * them (in 4 MiB pieces, each on the link while the caller's thread copies the next) and
 * launches K1 asynchronously.  Non-blocking: a full ring drops the batch, counts it
 * and returns SG_EAGAIN (the reference's PersistRequest would block here, backend.go:844).      */
int sg_ingest(sg_handle h, const sg_event* events, size_t n);

/* The same without the staging copy, for events that already sit in page-locked host memory the caller registered with
 * sg_host_register (a C-allocated buffer a packer writes into; NOT Go-heap memory): the records are read asynchronously (H2D copy,
 * then K1 pass A) and must stay unchanged until sg_flush_end* / sg_flush_window* of their window has RETURNED (sg_flush_begin and
 * sg_window_run only enqueue: after sg_window_run synchronise its stream first).  Non-blocking like sg_ingest (SG_EAGAIN when no device
 * slot is free); SG_EINVAL when the events are not inside registered memory.                                              */
int sg_host_register(sg_handle h, void* p, size_t bytes);
int sg_host_unregister(sg_handle h, void* p);
int sg_ingest_pinned(sg_handle h, const sg_event* events, size_t n);
/* Blocking convenience for loaders that would rather wait than drop (replay tools, benchmarks): n events in max_batch-sized
 * pieces through sg_ingest (pinned = 0) or sg_ingest_pinned (pinned = 1); a full ring is waited for, not counted as a drop.
 * *retries (may be NULL) = how often it had to wait.  The aggregator-facing entry points above stay non-blocking.        */
int sg_ingest_bulk(sg_handle h, const sg_event* events, size_t n, int pinned, uint64_t* retries);

/* Same, for events already resident in device memory (bench, sharded feeder).  `stream` is a
 * hipStream_t (NULL = the engine's own stream); K1 is ordered after prior work of that stream. */
int sg_ingest_device(sg_handle h, const sg_event* d_events, size_t n, void* stream);

/* ---- window close ------------------------------------------------------------------------ *
 * One call for the unsharded case: K2..K5, copy-out, reset.  `out` receives up to `cap` rows,
 * *n the number of edges of the window (may exceed cap; then only cap rows were written).       */
int sg_flush_window(sg_handle h, uint64_t window_end_ms, sg_edge_out* out, size_t cap, size_t* n);

/* The same window close without the copy into caller memory: the rows are transferred into page-locked host memory the
 * engine owns and *rows points at them — valid until the next sg_flush_window / sg_flush_window_view / sg_window_read on
 * this handle, or sg_destroy.  *n = edges of the window (all of them are there).  For callers that only walk the rows once
 * (a Go shim building its payload, GraphDS::FlushWindow): a pageable 64 MB destination costs more than the transfer. */
int sg_flush_window_view(sg_handle h, uint64_t window_end_ms, const sg_edge_out** rows, size_t* n);

/* ---- selection (K7): only the window's most anomalous rows leave the device ---------------------------------------------- *
 * Candidates are the rows with score >= min_score (a plain float comparison: a NaN score is never one; -INFINITY admits every
 * other row).  k == 0: every candidate, in canonical order.  1 <= k <= SG_SELECT_MAX_K: the min(k, candidates) highest-scoring
 * candidates, descending by score, equal scores (-0.0 == +0.0) by ascending canonical position.  k > SG_SELECT_MAX_K: SG_EINVAL
 * before anything is enqueued or any window is closed.  Each row is byte-identical to the one sg_flush_window returns at that
 * position; row_index[j] (may be NULL) = that position.  *n_selected = rows selected (may exceed cap; then only cap rows and
 * indices were written), *n_edges = edges of the window.  The engine's state afterwards — sg_stats, sg_window_outbound_ips,
 * sg_window_hist, the kept warm state — is exactly what a plain flush of the window leaves.                                      */
#define SG_SELECT_MAX_K 16384u
int sg_flush_window_top(sg_handle h, uint64_t window_end_ms, uint32_t k, float min_score,
                        sg_edge_out* out, uint32_t* row_index, size_t cap, size_t* n_selected, size_t* n_edges);
/* sg_flush_end with the selection: ends the window sg_flush_begin closed.                                                    */
int sg_flush_end_top(sg_handle h, uint32_t k, float min_score,
                     sg_edge_out* out, uint32_t* row_index, size_t cap, size_t* n_selected, size_t* n_edges);
/* Device-resident form for sg_window_run drivers: selects from the rows sg_window_rows_buffer names (the window sg_window_run
 * closed last, whichever slot it ran on) into caller-owned device memory — d_out [cap] rows, d_index [cap] u32 (may be NULL),
 * *d_n (u64) = rows selected — enqueued on `stream` (NULL = the stream that window ran on), no host sync.  Enqueue it behind that
 * window's sg_window_run and before the slot's next ingest.                                                                   */
int sg_window_select(sg_handle h, uint32_t k, float min_score, sg_edge_out* d_out, uint32_t* d_index,
                     size_t cap, uint64_t* d_n, void* stream);

/* ---- per-edge baselines (K8): each edge against its own past, kept on the device across windows --------------------------- *
 * Opt-in (sg_set_trend); an engine without it computes and allocates nothing for it, and its rows are the same either way.
 * Edge key: from_key, to_key = type << 32 | v with type = SG_REF_TYPE(ref), v = SG_REF_VALUE(ref) for KNOWN / LABEL refs and the
 * IPv4 address (the window's outbound-IP list at SG_REF_VALUE(ref)) for OBIP refs.  The canonical row order is strictly
 * ascending in (from_key, to_key), and the baseline is kept sorted by it: each window is a merge of two sorted lists.
 * Sample of a row with count > 0 (rows with count == 0 — alive-only edges — neither create nor refresh an entry), exact in fp64:
 *   x_lat = min(sum_ns / count, 2^52), x_err = (err_count << 20) / count   (u64 integer divisions; err in units of 2^-20)
 * Entry update in trend window w (w counts the windows closed while the trend is on, from 1; alpha = 2^-shift): a new entry gets
 * mean = x, dev = 0, n = 1, last = w; an existing one d = x - mean, mean += d * alpha, dev += (|d| - dev) * alpha, n = min(n + 1,
 * 2^32 - 1), last = w (latency and error alike).  Every product is exact: the state equals a float64 reference bit for bit.  An
 * entry NOT updated in window w with w - last >= ttl is removed.  Capacity: the kept old entries never exceed max_entries; new
 * ones go in in key order while there is room, the rest are dropped and counted.
 * Per row, from the entry as it was BEFORE the window's update: windows_seen = its n (0: never seen, expired or dropped — with
 * count > 0 a new dependency); lat_dev = (float)((x_lat - lat_mean) / max(lat_dev, lat_floor_ns)), 0 when count == 0 or
 * windows_seen < warmup; err_dev likewise with err_floor; base_mean_us = (float)(lat_mean / 1000), 0 without an entry.          */
typedef struct sg_trend_params {
    uint32_t struct_size;       /* sizeof(sg_trend_params)                                                                  */
    uint32_t shift;             /* alpha = 2^-shift, 1..10 (0 = 4)                                                           */
    uint32_t warmup;            /* windows an entry must have seen before its rows report deviations (0 = 4)                 */
    uint32_t ttl;               /* windows an entry survives without a sample (0 = 64)                                       */
    uint64_t max_entries;       /* baseline capacity, at most 2^31 (0 = 2 x max_edges)                                       */
    uint64_t lat_floor_ns;      /* latency deviation floor (0 = 1000)                                                        */
    uint32_t err_floor;         /* error deviation floor in units of 2^-20 (0 = 10486, 1 %)                                  */
    uint32_t reserved;          /* 0                                                                                         */
} sg_trend_params;
typedef struct sg_edge_trend { float lat_dev, err_dev, base_mean_us; uint32_t windows_seen; } sg_edge_trend;
typedef struct sg_trend_entry { uint64_t from_key, to_key; double lat_mean, lat_dev, err_mean, err_dev; uint32_t n, last; } sg_trend_entry;
typedef struct sg_trend_stats {
    uint64_t windows;           /* windows the baseline was updated by since it was (re)enabled                              */
    uint64_t entries;           /* entries now                                                                               */
    uint64_t inserted, expired, dropped;   /* totals since it was (re)enabled                                                */
} sg_trend_stats;
/* NULL = off (frees the baseline); params = on, and (re)enabling starts an empty baseline.  Buffers are allocated here, not at
 * create.  SG_ESTATE while a flush is open, SG_EINVAL on bad params.  Trend calls on an engine without the trend: SG_ESTATE. */
int sg_set_trend(sg_handle h, const sg_trend_params* p);
/* The trend rows of the last READ window (the rows sg_flush_window* / sg_window_read returned; all zero for a window closed before
 * the trend was enabled).  row_index NULL: every row, *n = edges; else out[k] = the trend of row row_index[k] (each < edges, else
 * SG_EINVAL), *n = n_index — only those n_index entries cross PCIe.  min(*n, cap) entries are written.                         */
int sg_window_trend(sg_handle h, const uint32_t* row_index, size_t n_index, sg_edge_trend* out, size_t cap, size_t* n);
/* Device sg_edge_trend[E] of the window sg_window_run / sg_window_run_sharded closed last (valid until its slot is reused; read it
 * on that window's stream).                                                                                                   */
int sg_window_trend_buffer(sg_handle h, void** d_trend);
/* The baseline in key order: min(*n, cap) entries, *n = entries (waits for the updates enqueued so far).                        */
int sg_trend_entries(sg_handle h, sg_trend_entry* out, size_t cap, size_t* n);
int sg_trend_stats_get(sg_handle h, sg_trend_stats* out);   /* (waits for the updates enqueued so far) */

/* Vanished dependencies: the baseline entries that stopped getting samples.  Opt-in (sg_set_vanished, on an engine with the trend);
 * the trend's rows and entries are the same either way.  In trend window w an OLD entry (one that was in the baseline before the
 * window) is vanished when all of these hold:
 *   - no row of the window with its key and count > 0 refreshes it;
 *   - its n >= min_seen;
 *   - w - last == silent_windows.
 * So an entry is reported once per silence, in the silent_windows-th window without a sample, and again if it comes back and goes
 * silent again.  New entries the capacity cut dropped were never old entries: they are never reported.  silent_windows < ttl, so a
 * reported entry has not expired: its fields are the entry as it stands after the window (unchanged by it).  row = the position of
 * the window's alive-only row (count == 0) with the entry's key, 0xFFFFFFFF when the window has no row with it.
 * The list of a window is in ascending key order (the merge order); *n counts every vanished entry of the window, and the first
 * min(*n, max_rows, cap) in key order are written.                                                                             */
typedef struct sg_vanished_params {
    uint32_t struct_size;       /* sizeof(sg_vanished_params)                                                                 */
    uint32_t silent_windows;    /* 1 .. ttl - 1 (0 = 1)                                                                       */
    uint32_t min_seen;          /* windows an entry must have seen (0 = the trend's warmup)                                   */
    uint32_t max_rows;          /* rows kept per window, 1 .. max_entries (0 = min(65536, max_entries))                       */
} sg_vanished_params;
typedef struct sg_edge_vanished {
    uint64_t from_key, to_key;                      /* K8's edge key                                                         */
    double   lat_mean, lat_dev, err_mean, err_dev;  /* the entry as it stands after the window                                */
    uint32_t n, last;                               /* windows seen; trend window of its last sample                          */
    uint32_t row;                                   /* this window's alive-only row with the key, else 0xFFFFFFFF              */
    uint32_t reserved;                              /* 0                                                                      */
} sg_edge_vanished;             /* 64 bytes, no padding */
/* NULL = off (frees the lists); params = on: the per-slot lists are allocated here, never at create.  SG_ESTATE when the trend is
 * off or a flush is open, SG_EINVAL on bad params.  Any sg_set_trend call switches the vanished list off and frees it.           */
int sg_set_vanished(sg_handle h, const sg_vanished_params* p);
/* The vanished list of the last READ window (as sg_window_nodes).  SG_ESTATE for a window closed while the list was off, and while
 * a flush is open.                                                                                                              */
int sg_window_vanished(sg_handle h, sg_edge_vanished* out, size_t cap, size_t* n);
/* Device sg_edge_vanished[max_rows] and its count (one uint64_t) of the window sg_window_run / sg_window_run_sharded closed last
 * (valid until its slot is reused; read them on that window's stream).                                                         */
int sg_window_vanished_buffer(sg_handle h, void** d_rows, void** d_count);

/* Selection (K7) by a trend key: the K7 semantics with the score replaced by the chosen value of the row's sg_edge_trend — a plain
 * float comparison value >= min_value (NaN never), k = 0 every candidate in canonical order, 1 <= k <= SG_SELECT_MAX_K the highest
 * values descending, ties (-0.0 == +0.0) by row position.  SG_SEL_NEW: the candidates are the rows with windows_seen == 0 and
 * count > 0, all with the same key (min_value ignored): k > 0 gives the first k new edges in canonical order.  Rows are byte-identical
 * to the plain flush's; row_index can be passed straight to sg_window_trend.  by > 3: SG_EINVAL; a trend key on an engine without the
 * trend: SG_ESTATE — both before any window is closed.  by = SG_SEL_SCORE is the plain selection (same bytes).                   */
#define SG_SEL_SCORE   0u   /* = sg_flush_window_top and friends                                                              */
#define SG_SEL_LAT_DEV 1u   /* sg_edge_trend.lat_dev of the row                                                               */
#define SG_SEL_ERR_DEV 2u   /* sg_edge_trend.err_dev of the row                                                               */
#define SG_SEL_NEW     3u   /* rows with windows_seen == 0 and count > 0; min_value ignored                                   */
int sg_flush_window_top_by(sg_handle h, uint64_t window_end_ms, uint32_t by, uint32_t k, float min_value,
                           sg_edge_out* out, uint32_t* row_index, size_t cap, size_t* n_selected, size_t* n_edges);
int sg_flush_end_top_by(sg_handle h, uint32_t by, uint32_t k, float min_value,
                        sg_edge_out* out, uint32_t* row_index, size_t cap, size_t* n_selected, size_t* n_edges);
/* sg_window_select by a trend key: the trend rows of the window sg_window_rows_buffer names.                                    */
int sg_window_select_by(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_edge_out* d_out, uint32_t* d_index,
                        size_t cap, uint64_t* d_n, void* stream);

/* ---- node rollup (K9): each window's scored edges reduced per node, on the device ------------------------------------------ *
 * Opt-in (sg_set_nodes); an engine without it computes and allocates nothing for it, and its rows are the same either way.
 * Over the window's rows r_0 .. r_{E-1} in canonical order, the node set is every from_ref and to_ref of some row.  Node rows come
 * out ascending by (SG_REF_TYPE(ref), SG_REF_VALUE(ref)): KNOWN by id, then LABEL, then OBIP by index into the window's
 * outbound-IP list.  For node x the out_* fields reduce over the rows with from_ref == x, the in_* fields over the rows with
 * to_ref == x; a row with from_ref == to_ref counts on both sides.
 *   *_edges        rows                                 *_count, *_err     sum of count, err_count
 *   *_sum_ns, *_sumsq_us   wrapping u64 sums            *_max_ns           max of max_ns (0 without rows)
 *   *_alive        sum of alive                         *_score_q32        wrapping u64 sum of (uint64_t)((double)score * 2^32)
 *                                                                          (a score that is not > 0 adds 0): exact, order-free
 *   *_score_max    the largest score (0 without rows)   *_worst_row        the smallest row index among the side's rows whose
 *                                                                          score equals *_score_max (0xFFFFFFFF without rows)
 *   score          max(out_score_max, in_score_max)
 * Scores are compared by value with +0.0 above -0.0 (the window's scores are sigmoids in [0, 1]).  Every field is an integer sum, an
 * integer max or a max of floats: the result has one correct value, and each field merges across shards by sum or max.  The row
 * indices are the positions of sg_flush_window*, sg_flush_window_top's row_index and sg_window_trend's row_index.            */
typedef struct sg_node_out {
    uint64_t out_count, in_count, out_err, in_err, out_sum_ns, in_sum_ns, out_sumsq_us, in_sumsq_us, out_max_ns, in_max_ns,
             out_score_q32, in_score_q32;
    uint32_t ref, out_edges, in_edges, out_alive, in_alive, out_worst_row, in_worst_row;
    float    out_score_max, in_score_max, score;
} sg_node_out;                  /* 136 bytes, no padding */
/* on = 1: allocate the per-slot node buffers (a no-op when on); on = 0: free them.  SG_ESTATE while a flush is open, SG_EINVAL on
 * an engine with world > 1.  Node calls on an engine without the rollup: SG_ESTATE.                                            */
int sg_set_nodes(sg_handle h, int on);
/* The node rows of the last READ window (the window whose rows sg_flush_window* / sg_window_read returned): *n = nodes, min(*n, cap)
 * rows are written (a window without rows: *n = 0).  SG_ESTATE for a window closed while the rollup was off, and while a flush is
 * open (its window is being rolled up into the same buffer).                                                                  */
int sg_window_nodes(sg_handle h, sg_node_out* out, size_t cap, size_t* n);
/* Device sg_node_out[] and its count (one uint64_t) of the window sg_window_run closed last (valid until its slot is reused; read
 * them on that window's stream).                                                                                              */
int sg_window_nodes_buffer(sg_handle h, void** d_nodes, void** d_count);

/* ---- node baselines (K10) and node selection: each service against its own past, on the device ----------------------------- *
 * Opt-in (sg_set_node_trend, on an engine with the node rollup); without it nothing is computed or allocated, and the edge rows,
 * node rows, edge trend and vanished lists are the same either way.  K8's baseline kept per node side instead of per edge:
 * node key nk = type << 32 | x with K8's rule for one ref (x = SG_REF_VALUE(ref), the IPv4 address for OBIP refs); each node has
 * two entries, (from_key, to_key) = (nk, 0) "in" (the requests it received: in_count, in_err, in_sum_ns) and (nk, 1) "out" (the
 * requests it sent: out_*).  Node rows are ascending by ref and the outbound-IP list is ascending, so a window's samples are
 * strictly ascending in (nk, side) and an OBIP node keeps its baseline when its index in the list changes.
 * Sample of a side with count c > 0 (u64), sum s (the node row's wrapping u64 *_sum_ns) and errors e, exact in fp64:
 *   x_lat = min(floor(s / c), 2^52), x_err = floor(e * 2^20 / c)   (exact: the product does not overflow)
 * A side with c == 0 neither creates nor refreshes an entry.  The entry update, expiry and capacity cut are K8's word for word,
 * with sg_trend_params (max_entries 0 = min(2^31, 4 x the engine's node capacity)) and a trend-window counter of its own.
 * Row k of a window's sg_node_trend belongs to node row k of sg_window_nodes; each side is K8's row rule from that side's entry as
 * it stood BEFORE the window's update: *_seen = its n; *_lat_dev / *_err_dev are 0 when the side's count is 0 or *_seen < warmup;
 * *_base_mean_us = (float)(lat_mean / 1000), 0 without an entry.  Every close path updates it (one call, begin + end,
 * sg_window_run); with several windows in flight the updates run in window order.                                            */
typedef struct sg_node_trend {
    float    in_lat_dev, in_err_dev, out_lat_dev, out_err_dev;
    float    in_base_mean_us, out_base_mean_us;
    uint32_t in_seen, out_seen;
} sg_node_trend;                /* 32 bytes, no padding */
/* NULL = off (frees the baseline); params = on, and (re)enabling starts an empty baseline.  Memory is allocated here, never at
 * create.  SG_ESTATE when the node rollup is off or a flush is open, SG_EINVAL on bad params.  sg_set_nodes(h, 0) switches it
 * off too; sg_set_trend does not touch it, nor it the edge trend.  Node trend calls on an engine without it: SG_ESTATE.        */
int sg_set_node_trend(sg_handle h, const sg_trend_params* p);
/* The node trend rows of the last READ window (as sg_window_nodes).  node_index NULL: every node row, *n = nodes; else out[k] =
 * the row of node node_index[k] (each < nodes, else SG_EINVAL), *n = n_index.  min(*n, cap) rows are written.  SG_ESTATE for a
 * window closed while the node trend was off, and while a flush is open.                                                     */
int sg_window_node_trend(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
/* Device sg_node_trend[] of the window sg_window_run closed last (its count is sg_window_nodes_buffer's; valid until the slot is
 * reused; read it on that window's stream).                                                                                  */
int sg_window_node_trend_buffer(sg_handle h, void** d_trend);
/* The node baseline in key order (to_key = side): min(*n, cap) entries, *n = entries (waits for the updates enqueued so far).    */
int sg_node_trend_entries(sg_handle h, sg_trend_entry* out, size_t cap, size_t* n);
int sg_node_trend_stats_get(sg_handle h, sg_trend_stats* out);   /* (waits for the updates enqueued so far) */

/* Node selection (K7 over node rows): the K7 semantics with "row" read as "node row" and the key chosen by `by` — a plain float
 * comparison value >= min_value (NaN never), k = 0 every candidate in node order, 1 <= k <= SG_SELECT_MAX_K the highest values
 * descending, ties (-0.0 == +0.0) by node position.  SG_NSEL_NEW: the nodes with in_seen == 0, out_seen == 0 and a request on
 * either side, all with one key (min_value ignored): k > 0 gives the first k in node order.  Rows are byte-identical to
 * sg_window_nodes's; node_index[j] (may be NULL) = that position, to pass straight to sg_window_node_trend.  by > 5 or
 * k > SG_SELECT_MAX_K: SG_EINVAL; the node rollup off, or a trend key with the node trend off: SG_ESTATE.                    */
#define SG_NSEL_SCORE       0u  /* sg_node_out.score (needs only the rollup) */
#define SG_NSEL_IN_LAT_DEV  1u
#define SG_NSEL_IN_ERR_DEV  2u
#define SG_NSEL_OUT_LAT_DEV 3u
#define SG_NSEL_OUT_ERR_DEV 4u
#define SG_NSEL_NEW         5u  /* in_seen == 0 && out_seen == 0 && in_count + out_count > 0; min_value ignored */
/* Over the node rows of the last READ window, on the engine's read stream; returns when done.  *n_selected = nodes selected (may
 * exceed cap; then only cap rows and indices were written), *n_nodes = nodes of the window.  SG_ESTATE also for a window closed
 * while the rollup (or, for a trend key, the node trend) was off, and while a flush is open.                                  */
int sg_window_nodes_top(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out,
                        uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);
/* Device-resident form over the window sg_window_run closed last: d_out [cap] node rows (may be NULL), d_index [cap] u32 (may be
 * NULL), *d_n (u64) = nodes selected, enqueued on `stream` (NULL = the stream that window ran on), no host sync.                */
int sg_window_nodes_select(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* d_out,
                           uint32_t* d_index, size_t cap, uint64_t* d_n, void* stream);

/* ---- culprit ranking (K11): each window's likely root-cause services, by a walk over the window's own graph, on the device ---- *
 * Opt-in (sg_set_rank, on an engine with the node rollup); without it nothing is computed or allocated, and every other row is
 * the same either way.  A random walk with restart over the window's rows, stepping from caller to callee with probability
 * proportional to the row's anomaly: mass drains downstream along anomalous rows and piles up where they stop.  Integer
 * arithmetic only (u64, every intermediate below 2^64), so the result has one correct value.
 * Over the window's rows j = 0 .. E-1 (canonical order) and its node rows v = 0 .. n-1 (sg_window_nodes order):
 *   q16(s)  = s > 0 ? min((uint32_t)(s * 65536.0f), 65536) : 0      (NaN: 0; the product is exact, the conversion truncates)
 *   w_j     = 1 + q16(score_j) for every row (alive-only rows too);  W_u = sum of w_j over the rows with from_ref == u
 *   seed    SG_RANK_SEED_SCORE: a_v = node.score >= seed_min_score ? q16(node.score) : 0;  SG_RANK_SEED_UNIFORM: a_v = 1;
 *           A = sum of a_v; A == 0: the seed falls back to uniform (a_v = 1, A = n)
 *   M = 2^56;  p_v = a_v * floor(M / A);  D = damping_q8 in 1..255 (0 = 218, i.e. 0.85);  R_v = (p_v >> 8) * (256 - D);  r_v = p_v
 *   one iteration, `iters` times (1..64, 0 = 20; a fixed count, no convergence test):
 *           m_u = (r_u >> 8) * D;  t_u = W_u ? floor(m_u / W_u) : 0;
 *           r'_v = R_v + (m_v - t_v * W_v) + sum over the rows j with to_ref == v of t_{from_j} * w_j
 *           (what the division does not hand out stays at u; a node without out-rows keeps all of m_u: it is a sink, where the
 *           walk ends; a row with from_ref == to_ref is an ordinary row)
 *   row v   rank = r_v after the last iteration, ref = the node row's ref, share = (float)((double)rank * 2^-56)
 * Invariants: sum r' == sum R + sum m exactly, and sum r <= M; hence r_u <= 2^56, (r_u >> 8) * 255 < 2^56, t_u * w_j <= m_u, and
 * W_u <= 65537 * E.  Selection (K7 over the rank rows): key min(rank >> 24, 0xFFFFFFFF), key 0 is not a candidate, share >=
 * min_share as a plain float comparison (NaN never), k = 0 every candidate in node order, 1 <= k <= SG_SELECT_MAX_K the highest
 * keys descending, ties by node position.  Every close path computes it (one call, begin + end, sg_window_run).              */
#define SG_RANK_SEED_SCORE   0u
#define SG_RANK_SEED_UNIFORM 1u
typedef struct sg_rank_params {
    uint32_t struct_size;       /* sizeof(sg_rank_params)                                       */
    uint32_t iters;             /* 1..64; 0 = 20                                                */
    uint32_t damping_q8;        /* 1..255; 0 = 218                                              */
    uint32_t seed;              /* SG_RANK_SEED_*                                               */
    float    seed_min_score;    /* SG_RANK_SEED_SCORE: nodes below it seed nothing              */
    uint32_t reserved;          /* 0                                                            */
} sg_rank_params;               /* 24 bytes */
typedef struct sg_node_rank {
    uint64_t rank;
    uint32_t ref;
    float    share;
} sg_node_rank;                 /* 16 bytes, no padding */
/* NULL = off (frees its memory); params = on.  Memory is allocated here, never at create.  SG_ESTATE when the node rollup is off
 * or a flush is open, SG_EINVAL on bad params.  sg_set_nodes(h, 0) switches it off too.  Rank calls on an engine without it:
 * SG_ESTATE.                                                                                                                 */
int sg_set_rank(sg_handle h, const sg_rank_params* p);
/* The rank rows of the last READ window (as sg_window_node_trend): node_index NULL: every node row, *n = nodes; else out[k] = the
 * row of node node_index[k] (each < nodes, else SG_EINVAL), *n = n_index.  min(*n, cap) rows are written.  SG_ESTATE for a window
 * closed while the ranking was off, and while a flush is open.                                                               */
int sg_window_rank(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_rank* out, size_t cap, size_t* n);
/* Device sg_node_rank[] of the window sg_window_run closed last (its count is sg_window_nodes_buffer's; valid until the slot is
 * reused; read it on that window's stream).                                                                                  */
int sg_window_rank_buffer(sg_handle h, void** d_rank);
/* Selection over the rank rows of the last READ window, on the engine's read stream; returns when done.  out [cap] node rows
 * (byte-identical to sg_window_nodes's), rank_out [cap] their rank rows, node_index [cap] their positions (each may be NULL);
 * *n_selected = nodes selected (may exceed cap), *n_nodes = nodes of the window.  k > SG_SELECT_MAX_K: SG_EINVAL.             */
int sg_window_rank_top(sg_handle h, uint32_t k, float min_share, sg_node_out* out, sg_node_rank* rank_out,
                       uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);
/* Device-resident form over the window sg_window_run closed last: d_out [cap] node rows (may be NULL), d_index [cap] u32 (may be
 * NULL), *d_n (u64) = nodes selected, enqueued on `stream` (NULL = the stream that window ran on), no host sync.                */
int sg_window_rank_select(sg_handle h, uint32_t k, float min_share, sg_node_out* d_out, uint32_t* d_index,
                          size_t cap, uint64_t* d_n, void* stream);

/* ---- incidents (K12): each window's anomalous rows grouped into connected components, on the device ------------------------- *
 * Opt-in (sg_set_incidents, on an engine with the node rollup); without it nothing is computed or allocated, and every other row
 * is the same either way.  Over the window's rows j = 0 .. E-1 (canonical order) and its node rows v = 0 .. n-1 (sg_window_nodes
 * order):
 *   value_j  `by` = SG_SEL_SCORE: the row's score; SG_SEL_LAT_DEV / SG_SEL_ERR_DEV: this window's sg_edge_trend.lat_dev / .err_dev
 *            of the row (what sg_flush_window_top_by selects by)
 *   red      row j is red iff value_j >= min_value (a plain float comparison, NaN never) and both its from_ref and its to_ref
 *            have a node row (a ref beyond the engine's id spaces has none: K11 gives such a row weight 0); alive-only rows are
 *            ordinary rows
 *   graph    undirected, on the node rows, one edge {from, to} per red row.  A node row is in an incident iff it is an endpoint
 *            of a red row (a red row with from_ref == to_ref makes its node an incident on its own); the incidents are the
 *            connected components of those nodes, numbered 0 .. I-1 by ascending first_node, their smallest node row
 * Incident i:
 *   first_node, nodes    its smallest node row; its node rows
 *   edges                its red rows (other rows between its nodes do not count)
 *   count, err, sum_ns   wrapping u64 sums of the red rows' count, err_count, sum_ns
 *   score_q32            K9's sum of (uint64_t)((double)score * 2^32) over the red rows (a score that is not > 0 adds 0)
 *   value_max, worst_row the largest value among its red rows, +0.0 above -0.0; the smallest row index that has it
 *   top_node             the node row with the largest sg_node_out.score among its nodes (by the order-preserving bits of the
 *                        score, +0.0 above -0.0), ties to the smallest index
 *   culprit_node         with the ranking (K11) on for the window: the node row with the largest sg_node_rank.rank, ties to the
 *   rank_sum             smallest index; the wrapping u64 sum of its nodes' rank.  Ranking off: SG_NO_INCIDENT and 0
 * Every field is an integer sum, an integer max or a max of order-preserving float bits: the result has one correct value.
 * Every close path computes it (one call, begin + end, the views, the _top flushes, sg_window_run), behind K8, K9 and K11.   */
#define SG_NO_INCIDENT 0xFFFFFFFFu
typedef struct sg_incident_params {
    uint32_t struct_size;       /* sizeof(sg_incident_params)                                   */
    uint32_t by;                /* SG_SEL_SCORE, SG_SEL_LAT_DEV or SG_SEL_ERR_DEV; else SG_EINVAL */
    float    min_value;         /* a row is red iff its value >= min_value                      */
    uint32_t reserved;          /* 0                                                            */
} sg_incident_params;           /* 16 bytes */
typedef struct sg_incident_out {
    uint64_t count, err, sum_ns, score_q32, rank_sum;
    uint32_t first_node, nodes, edges, worst_row, top_node, culprit_node;
    float    value_max;
    uint32_t reserved;          /* 0 */
} sg_incident_out;              /* 72 bytes, no padding */
/* NULL = off (frees its memory); params = on.  Memory is allocated here, never at create.  SG_ESTATE when the node rollup is off,
 * a flush is open, or `by` is a trend key and the edge trend is off; SG_EINVAL on bad params.  sg_set_nodes(h, 0) switches it off
 * too; sg_set_trend(h, NULL) does so only when `by` is a trend key.  Incident calls on an engine without it: SG_ESTATE.        */
int sg_set_incidents(sg_handle h, const sg_incident_params* p);
/* The incidents of the last READ window (as sg_window_nodes): *n = incidents, min(*n, cap) rows are written.  SG_ESTATE for a
 * window closed while the stage was off, and while a flush is open.                                                          */
int sg_window_incidents(sg_handle h, sg_incident_out* out, size_t cap, size_t* n);
/* The incident number of every node row of the last READ window, SG_NO_INCIDENT for a node in none (as sg_window_rank):
 * node_index NULL: every node row, *n = nodes; else out[k] = the number of node node_index[k] (each < nodes, else SG_EINVAL),
 * *n = n_index.  min(*n, cap) values are written.  SG_ESTATE as sg_window_incidents.                                          */
int sg_window_node_incident(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
/* Device sg_incident_out[], their count (one uint64_t) and uint32_t[nodes] (the incident per node row) of the window
 * sg_window_run closed last (valid until its slot is reused; read them on that window's stream).                              */
int sg_window_incidents_buffer(sg_handle h, void** d_incidents, void** d_count, void** d_node_incident);

/* ---- tracks (K13): each window's incidents followed across windows, on the device -------------------------------------------- *
 * Opt-in (sg_set_tracks, on an engine with the incidents); without it nothing is computed or allocated, and every other row is the
 * same either way.  A track is an incident followed over time: every incident of every window belongs to exactly one track, and a
 * track's id never changes and is never reused.  w = the windows closed since sg_set_tracks switched tracking on (the first: 0).
 * Over the window's node rows v (sg_window_nodes order), its incidents i = 0 .. I-1 and inc[v] (sg_window_node_incident):
 *   anchor   a node row whose ref is KNOWN or LABEL (those refs mean the same thing in every window; an OBIP ref is an index into
 *            the window's own outbound-IP list: such a node rides with its incident and carries no membership).  Every row has a
 *            pod at one end, so every incident has an anchor.
 * Kept state:
 *   member   per anchor ref (track, last): the track of the incident the ref was in most recently, and that window's w
 *   table    ascending by id, sg_track_entry {track, parent, first_window, last_window, windows, peak_nodes, count, err}
 *   live     an entry with last_window = L is live at w iff w - L - 1 <= quiet_windows; a member (T, l) is live at w iff
 *            w - l - 1 <= quiet_windows and the table holds a live entry T.  t_v = the track of v's live member; SG_NO_TRACK for a
 *            node without one and for every node that is no anchor
 * Per window, in this order:
 *   1  cand_i = the smallest t_v over the nodes of incident i (ids ascend in time: the oldest track), SG_NO_TRACK if there is none
 *   2  over the anchors of i: kept_i = those with t_v == cand_i != SG_NO_TRACK; moved_i = those with t_v != SG_NO_TRACK and
 *      t_v != cand_i; joined_i = those with t_v == SG_NO_TRACK
 *   3  each track T goes to one claimant: among the incidents with cand_i == T the one with the largest kept_i, ties to the
 *      smallest i
 *   4  incident i continues cand_i if it is that track's claimant; otherwise it opens a track.  Ids of opened tracks are next_id +
 *      rank, the rank taken among the window's opening incidents in incident order; next_id then advances by their number.  The
 *      opened track's parent is cand_i (SG_NO_TRACK for an incident that touched no live track)
 *   5  entry: continued: last_window = w, windows += 1, peak_nodes = max(peak_nodes, nodes_i), count += count_i, err += err_i
 *      (wrapping u64, the incident row's fields); opened: {id, parent, w, w, 1, nodes_i, count_i, err_i}
 *   6  row i of sg_window_incident_tracks: {track, parent, first_window, windows (after the update), kept_nodes, moved_nodes,
 *      joined_nodes, flags}; SG_TRACK_NEW: opened this window; SG_TRACK_SPLIT: opened although cand_i != SG_NO_TRACK;
 *      SG_TRACK_MERGED: moved_i > 0
 *   7  every anchor of incident i gets member (track_i, w); other members stay as they are
 *   8  ended list of window w: the entries not continued at w whose last_window == w - 1, as they stood, in id order: a track is
 *      listed once, in its first silent window; a track absorbed by a merge is listed then too
 *   9  new table: the old entries that were continued or for which w - last_window <= quiet_windows, in id order, then the opened
 *      ones in incident order; only the first max_tracks positions are stored.  An opened track beyond them is still reported in
 *      this window's rows and consumes its id; it is not kept and is counted in dropped_cap.  A member that names an id the table
 *      lacks is not live.
 * Every field is an integer sum, an integer max, a min of ids or the max of a (count << 32 | ~index) key: the result has one
 * correct value.  Every close path computes it (one call, begin + end, the views, the _top flushes, sg_window_run), behind K12; with
 * several windows in flight the state updates run in window order.  w and the ids are 32 bits wide: re-enable tracking
 * (sg_set_tracks) before 2^32 - 1 windows were closed or ids were given out — at a window a millisecond, seven weeks — since
 * first_window and windows lose their meaning when w wraps, and an id must never reach SG_NO_TRACK.                            */
#define SG_NO_TRACK     0xFFFFFFFFu
#define SG_TRACK_NEW    1u
#define SG_TRACK_SPLIT  2u
#define SG_TRACK_MERGED 4u
#define SG_TRACK_MAX_QUIET 15u
typedef struct sg_track_params {
    uint32_t struct_size;       /* sizeof(sg_track_params)                                      */
    uint32_t quiet_windows;     /* 0..SG_TRACK_MAX_QUIET; 0: only the directly preceding window continues */
    uint32_t max_tracks;        /* table capacity; 0 = (quiet_windows + 1) * the rollup's node capacity: nothing is ever cut */
    uint32_t reserved;          /* 0                                                            */
} sg_track_params;              /* 16 bytes */
typedef struct sg_incident_track {
    uint32_t track, parent, first_window, windows, kept_nodes, moved_nodes, joined_nodes, flags;
} sg_incident_track;            /* 32 bytes */
typedef struct sg_track_entry {
    uint32_t track, parent, first_window, last_window, windows, peak_nodes;
    uint64_t count, err;
} sg_track_entry;               /* 40 bytes, no padding */
typedef struct sg_track_stats {
    uint64_t windows;           /* windows closed since tracking was (re)enabled                */
    uint64_t live;              /* entries in the table now                                     */
    uint64_t opened;            /* tracks opened since then (the next id)                       */
    uint64_t dropped_cap;       /* opened tracks the table had no room for                      */
} sg_track_stats;
/* NULL = off (frees its memory); params = on, and (re)enabling starts an empty state at w = 0, next id 0.  Memory is allocated
 * here, never at create.  SG_ESTATE when the incidents are off or a flush is open, SG_EINVAL on bad params.  Every
 * sg_set_incidents call, on or off, switches tracking off and frees it, and so does whatever switches the incidents off
 * (sg_set_nodes(h, 0), sg_set_trend(h, NULL) under a trend key).  Track calls on an engine without it: SG_ESTATE.               */
int sg_set_tracks(sg_handle h, const sg_track_params* p);
/* Row i belongs to incident i of the last READ window (as sg_window_incidents): *n = incidents, min(*n, cap) rows are written.
 * SG_ESTATE for a window closed while tracking was off, and while a flush is open.                                           */
int sg_window_incident_tracks(sg_handle h, sg_incident_track* out, size_t cap, size_t* n);
/* The ended list of the last READ window: *n = entries, min(*n, cap) are written.  SG_ESTATE as sg_window_incident_tracks.    */
int sg_window_tracks_ended(sg_handle h, sg_track_entry* out, size_t cap, size_t* n);
/* Device sg_incident_track[] (their count is sg_window_incidents_buffer's), the ended sg_track_entry[] and their count (one
 * uint64_t) of the window sg_window_run closed last (valid until its slot is reused; read them on that window's stream).        */
int sg_window_tracks_buffer(sg_handle h, void** d_tracks, void** d_ended, void** d_ended_count);
/* The live table in id order: min(*n, cap) entries, *n = entries (waits for the updates enqueued so far).                      */
int sg_track_entries(sg_handle h, sg_track_entry* out, size_t cap, size_t* n);
int sg_track_stats_get(sg_handle h, sg_track_stats* out);   /* (waits for the updates enqueued so far) */

/* ---- groups (K14): each window's service map contracted to workloads, on the device ------------------------------------------- *
 * Opt-in (sg_set_groups); without it nothing is computed or allocated, and every other row is the same either way.  It needs none
 * of K8 - K13 and changes none of them.  Every pod is its own node, so a Deployment of 20 replicas calling one service makes 20
 * rows; the host assigns KNOWN node ids to groups (workloads) and each window's rows are contracted to one row per (group, group).
 *   group map   group[id] in [0, max_groups) or SG_NO_GROUP (the initial value of every id, and again after every sg_set_groups);
 *               LABEL and OBIP nodes are never grouped
 *   group ref   of a node ref r: SG_MAKE_REF(SG_REF_GROUP, g) when r is KNOWN and group[SG_REF_VALUE(r)] = g != SG_NO_GROUP, else r
 *   group key   gk(r) = g for a grouped node, else max_groups + k with k = K9's node key of r: v (KNOWN), max_known_nodes + v
 *               (LABEL), max_known_nodes + max_labels + v (OBIP), v = SG_REF_VALUE(r).  gk < GK = max_groups + the engine's node
 *               capacity.  Ascending gk: the groups by id, then the ungrouped KNOWN nodes by id, then LABEL, then OBIP by index
 *   perm        over the window's rows r_0 .. r_{E-1} (canonical order): the permutation of 0 .. E-1 ascending by
 *               (gk(from_ref), gk(to_ref), row index) — one total order, so perm has exactly one correct value
 *   group edge  a maximal run of perm with equal (gk(from_ref), gk(to_ref)); the group edges come out in that order.  A run with
 *               gk(from) == gk(to) (traffic inside a workload) is an ordinary group edge
 * Group edge fields, over the rows of its run:
 *   count, err_count        u64 sums                        sum_ns, sumsq_us   wrapping u64 sums
 *   max_ns                  max                             alive              wrapping u32 sum
 *   score_q32, score_max, worst_row   K9's definitions: the wrapping u64 sum of (uint64_t)((double)score * 2^32) (a score that is
 *                           not > 0 adds 0); the largest score, +0.0 above -0.0; the smallest row index that has it
 *   from_ref, to_ref        the group refs of the rows' endpoints
 *   edges                   rows in the run (alive-only rows included)
 *   first                   the position in perm of the run's first row
 *   from_nodes              distinct from_ref in the run: the positions of the run that are its first, or whose row's from_ref
 *                           differs from the from_ref of the position before.  This counts distinct refs only because perm is
 *                           stable and the rows are sorted by from first: within a run the row indices ascend, so equal from_refs
 *                           are adjacent
 * row_group[j] = the index of the group edge row j belongs to.  Every field is an integer sum, an integer max or a max of a key:
 * the result has one correct value.  Every close path computes it (one call, begin + end, the views, the _top flushes,
 * sg_window_run, the staged sg_window_score), behind K5 (and K8 - K13 where they are on).                                     */
#define SG_REF_GROUP 3u         /* a workload: payload = the group id (sg_group_edge only)      */
#define SG_NO_GROUP  0xFFFFFFFFu
typedef struct sg_group_params {
    uint32_t struct_size;       /* sizeof(sg_group_params)                                      */
    uint32_t max_groups;        /* group ids are below it, at most 2^30; 0 = max_known_nodes    */
    uint32_t reserved[2];       /* 0                                                            */
} sg_group_params;              /* 16 bytes */
typedef struct sg_group_edge {
    uint64_t count, err_count, sum_ns, sumsq_us, max_ns, score_q32;
    uint32_t from_ref, to_ref;  /* group refs                                                   */
    uint32_t edges;             /* rows in the run (alive-only rows included)                   */
    uint32_t from_nodes;        /* distinct from_ref in the run                                 */
    uint32_t first;             /* position in perm of the run's first row                      */
    uint32_t alive;             /* wrapping u32 sum                                             */
    uint32_t worst_row;         /* smallest row index among the rows whose score == score_max  */
    float    score_max;
} sg_group_edge;                /* 80 bytes, no padding */
/* NULL = off (frees its memory); params = on.  Memory is allocated here, never at create.  Every call resets the map to "nothing
 * grouped".  SG_EINVAL on an engine with world > 1, a bad struct_size, non-zero reserved or max_groups > 2^30; SG_ESTATE while a
 * flush is open.  Group calls on an engine without it: SG_ESTATE.                                                              */
int sg_set_groups(sg_handle h, const sg_group_params* p);
/* group[node_ids[i]] = groups[i], i = 0 .. n-1 in that order.  SG_EINVAL for an id >= max_known_nodes or a group >= max_groups that
 * is not SG_NO_GROUP: then nothing is applied.  A window closed after the call returns is contracted under the new map; a window
 * closed before it is not, not even one still in flight on another slot.                                                       */
int sg_group_assign(sg_handle h, const uint32_t* node_ids, const uint32_t* groups, size_t n);
/* The group edges of the last READ window (as sg_window_incidents): *n = group edges, min(*n, cap) are written.  SG_ESTATE for a
 * window closed while the groups were off, and while a flush is open.                                                         */
int sg_window_groups(sg_handle h, sg_group_edge* out, size_t cap, size_t* n);
/* row_group of the last READ window (as sg_window_trend): row_index NULL: every row, *n = edges; else out[k] = row_group of row
 * row_index[k] (each < edges, else SG_EINVAL), gathered on the device, *n = n_index.  min(*n, cap) values are written.           */
int sg_window_row_group(sg_handle h, const uint32_t* row_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
/* perm of the last READ window: *n = edges, min(*n, cap) values are written.                                                    */
int sg_window_group_perm(sg_handle h, uint32_t* out, size_t cap, size_t* n);
/* Device sg_group_edge[], their count (one uint64_t), uint32_t row_group[edges] and uint32_t perm[edges] of the window
 * sg_window_run closed last (valid until its slot is reused; read them on that window's stream).                               */
int sg_window_groups_buffer(sg_handle h, void** d_edges, void** d_count, void** d_row_group, void** d_perm);

/* ---- workload baselines (K15): each group edge against its own past, vanished workload dependencies, selection ---------------- *
 * Opt-in (sg_set_group_trend), behind the groups; without it nothing is allocated or launched.  It needs none of K8 - K13 and
 * changes none of them.  K8's baseline is keyed by pod refs, so a rollout (new pods, new ids) makes every row of the workload a
 * "new dependency"; this one is keyed by workload and survives it.
 *   workload key  of a group ref r, a uint64_t: wk(r) = g when SG_REF_TYPE(r) == SG_REF_GROUP (key type 0); otherwise
 *                 wk(r) = (uint64_t)(1 + SG_REF_TYPE(r)) << 32 | x, x = SG_REF_VALUE(r), or the IPv4 address from the window's
 *                 outbound-IP list for an OBIP ref (the edge trend's key rule, one type up).  An OBIP endpoint keeps its entry when
 *                 its index in the list moves
 *   ordering      ascending wk is ascending gk: the groups by id, then the ungrouped KNOWN nodes by id, then LABEL, then OBIP — whose
 *                 index order is address order, the outbound-IP list being ascending.  A window's group edges come out ascending by
 *                 (gk(from), gk(to)) and no two share that pair, so they are STRICTLY ascending in (wk(from_ref), wk(to_ref)): the
 *                 window's samples are a sorted list, and the update is the edge trend's merge over them
 *   sample        of a group edge with count > 0, exact integers in fp64 (the counts are u64: the node baselines' two functions):
 *                 x_lat = min(floor(sum_ns / count), 2^52) on the wrapping u64 sum_ns; x_err = floor(err_count * 2^20 / count) by
 *                 long division (no overflow).  A group edge with count == 0 (it folds alive-only rows only) neither creates nor
 *                 refreshes an entry
 * Entry update, expiry, capacity cut and the per-sample output are the edge trend's, word for word; the parameters are
 * sg_trend_params with max_entries 0 = min(2^31, 2 x max_edges); the stage counts its own trend windows.  Row k of the output is
 * an sg_edge_trend for group edge k of sg_window_groups, from the entry as it stood before the window.
 * Vanished workload dependencies (sg_set_group_vanished) are sg_set_vanished's rule word for word over these entries:
 * sg_vanished_params, sg_edge_vanished rows with from_key / to_key workload keys and row = the index of the window's group edge
 * with the entry's key and count == 0, else 0xFFFFFFFF.
 * Selection is the row selection's semantics with "row" read as "group edge": by = SG_SEL_SCORE keys score_max of the group edge
 * (it needs the groups only), SG_SEL_LAT_DEV / SG_SEL_ERR_DEV its trend row's values, SG_SEL_NEW = windows_seen == 0 and count > 0;
 * ties go by group-edge position; the selected rows are byte-identical to sg_window_groups' and the indices can be passed to
 * sg_window_group_trend.
 * State: sg_set_group_trend is SG_ESTATE with the groups off or while a flush is open, SG_EINVAL on bad parameters; (re)enabling
 * starts an empty baseline; NULL = off.  ANY sg_set_groups call switches the group trend and its vanished list off and frees them
 * (it resets the map: the keys mean something else afterwards).  sg_group_assign does not touch the baseline: entries under keys
 * that no longer occur go silent, are listed once as vanished and expire by ttl.  Any sg_set_group_trend call switches the group
 * vanished list off.  Reads of a window closed while the stage was off: SG_ESTATE.                                               */
int sg_set_group_trend(sg_handle h, const sg_trend_params* p);
/* The group trend rows of the last READ window (as sg_window_trend): group_index NULL: every group edge, *n = group edges; else
 * out[k] = the row of group edge group_index[k] (each < group edges, else SG_EINVAL), gathered on the device, *n = n_index.       */
int sg_window_group_trend(sg_handle h, const uint32_t* group_index, size_t n_index, sg_edge_trend* out, size_t cap, size_t* n);
/* Device sg_edge_trend[group edges] of the window sg_window_run closed last (read it on that window's stream).                  */
int sg_window_group_trend_buffer(sg_handle h, void** d_trend);
/* The workload baseline in key order / its running statistics (both wait for the updates enqueued so far).                      */
int sg_group_trend_entries(sg_handle h, sg_trend_entry* out, size_t cap, size_t* n);
int sg_group_trend_stats_get(sg_handle h, sg_trend_stats* out);
/* NULL = off; SG_ESTATE with the group trend off or while a flush is open, SG_EINVAL on bad parameters (sg_set_vanished's rules
 * against the group trend's parameters).                                                                                        */
int sg_set_group_vanished(sg_handle h, const sg_vanished_params* p);
/* The vanished workload dependencies of the last READ window, ascending by key: *n = every vanished entry of the window (may
 * exceed max_rows), min(*n, cap, max_rows) are written.                                                                          */
int sg_window_group_vanished(sg_handle h, sg_edge_vanished* out, size_t cap, size_t* n);
int sg_window_group_vanished_buffer(sg_handle h, void** d_rows, void** d_count);
/* Selection over the group edges of the last READ window into host memory: min(*n_selected, cap) group edges to out and their
 * indices to group_index (either may be NULL), *n_selected = group edges selected (may exceed cap), *n_groups = group edges of the
 * window.  by > SG_SEL_NEW or k > SG_SELECT_MAX_K: SG_EINVAL; the groups off, a trend key with the group trend off, a window closed
 * without them, or an open flush: SG_ESTATE.                                                                                    */
int sg_window_groups_top(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_group_edge* out, uint32_t* group_index,
                         size_t cap, size_t* n_selected, size_t* n_groups);
/* The same over the window sg_window_run closed last, into device memory, enqueued on `stream` (NULL = that window's stream):
 * d_out [cap] group edges (may be NULL), d_index [cap] uint32_t (may be NULL), *d_n = group edges selected.                     */
int sg_window_groups_select(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_group_edge* d_out, uint32_t* d_index,
                            size_t cap, uint64_t* d_n, void* stream);

/* ---- workload rows (K16): the window's group edges rolled up per workload, their baselines and selection ---------------------- *
 * Opt-in (sg_set_group_nodes), behind the groups; without it nothing is allocated or launched.  It needs none of K8 - K13 or K15
 * and changes none of them.  There is no new struct and no new constant: the rows are sg_node_out, the trend rows sg_node_trend,
 * the entries sg_trend_entry, the parameters sg_trend_params, the selection keys SG_NSEL_*.
 *   node set   of a window: every from_ref and to_ref of its group edges — group refs: SG_REF_GROUP | g, or the node's own ref when
 *              it is ungrouped.  One sg_node_out per node
 *   order      ascending by the group key gk of sg_window_groups: the groups by id, then the ungrouped KNOWN nodes by id, then
 *              LABEL, then OBIP by index.  This is NOT ascending by the raw ref word: SG_REF_GROUP is type 3, and the groups come
 *              first
 *   fields     for node x the out_* fields reduce the group edges with from_ref == x, the in_* fields those with to_ref == x; a
 *              group edge inside a workload (from_ref == to_ref) counts on both sides.
 *                *_edges      the number of GROUP EDGES on that side (distinct peer workloads), not rows
 *                *_count, *_err, *_sum_ns, *_sumsq_us, *_score_q32
 *                             wrapping u64 sums of count, err_count, sum_ns, sumsq_us, score_q32
 *                *_max_ns     max of max_ns;   *_alive: wrapping u32 sum of alive
 *                *_score_max, *_worst_row
 *                             from the max of the 64-bit key (order-preserving key of score_max << 32 | ~worst_row) over the
 *                             side's group edges: the largest score among the underlying ROWS and the smallest row index that has
 *                             it — a row index of the window's rows, as in the node rollup; row_group[worst_row] names the group
 *                             edge.  A side without group edges: 0.0f and 0xFFFFFFFF
 *                score        max(out_score_max, in_score_max);   ref: the group ref
 *              Every field is an integer sum, an integer max or the max of a key: the result has one value, and it equals the node
 *              rollup's definition over the window's rows with each ref replaced by its group ref, but for *_edges and the order.
 * sg_set_group_nodes(h, 1 / 0): SG_ESTATE with the groups off or while a flush is open; SG_EINVAL when max_groups + the node
 * capacity (max_known_nodes + max_labels + max_obip) exceeds 2^21 group keys — pass a tighter max_groups to sg_set_groups: the
 * tables are per key (256 MB and 128 MB of partials at 2^21 keys).  It allocates here, never at sg_create or sg_set_groups.  ANY
 * sg_set_groups call frees this stage and everything behind it.  A window has at most min(2^21 keys, 2 x max_edges) rows.       */
int sg_set_group_nodes(sg_handle h, int on);
/* The workload rows of the last READ window: *n = rows of the window, min(*n, cap) are written (sg_window_nodes' rules).  SG_ESTATE
 * with the stage off, while a flush is open, or when that window was closed while the stage was off.                            */
int sg_window_group_nodes(sg_handle h, sg_node_out* out, size_t cap, size_t* n);
/* Device sg_node_out[] and its uint64_t count of the window sg_window_run closed last (valid until its slot is reused; read them
 * on that window's stream).                                                                                                     */
int sg_window_group_nodes_buffer(sg_handle h, void** d_nodes, void** d_count);
/* Baselines per workload and side: the node baselines word for word, with the key (wk(ref), side) — wk the workload key of the
 * group trend (the group id for a group, otherwise the edge trend's ref key one type up, the IPv4 address for an OBIP ref).
 * Ascending gk is ascending wk, so a window's 2 N samples (sample 2 k + side of row k, side 0 = in, 1 = out) are strictly ascending
 * and the update is the edge trend's merge.  max_entries 0 = min(2^31, 4 x the row capacity); the stage counts its own trend
 * windows; a side with count 0 neither creates nor refreshes an entry; sg_group_assign does not touch the baseline: a workload
 * keeps its entry through a rollout.  NULL = off; sg_set_group_nodes(h, 0) and any sg_set_groups call switch it off.  SG_ESTATE
 * with the workload rows off or while a flush is open, SG_EINVAL on bad parameters.                                             */
int sg_set_group_node_trend(sg_handle h, const sg_trend_params* p);
int sg_window_group_node_trend(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
int sg_window_group_node_trend_buffer(sg_handle h, void** d_trend);
int sg_group_node_trend_entries(sg_handle h, sg_trend_entry* out, size_t cap, size_t* n);
int sg_group_node_trend_stats_get(sg_handle h, sg_trend_stats* out);
/* Selection: sg_window_nodes_top / sg_window_nodes_select with "node row" read as "workload row" — the SG_NSEL_* keys, the tie rule
 * (by row position) and the error codes are the same; SG_NSEL_SCORE needs the workload rows only.  The selected rows are
 * byte-identical to sg_window_group_nodes' and the indices can be passed to sg_window_group_node_trend.                         */
int sg_window_group_nodes_top(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* node_index,
                              size_t cap, size_t* n_selected, size_t* n_nodes);
int sg_window_group_nodes_select(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* d_out, uint32_t* d_index,
                                 size_t cap, uint64_t* d_n, void* stream);

/* ---- workload ranking (K17): each window's likely root-cause workloads, by K11's walk over the contracted graph, on the device -- *
 * Opt-in (sg_set_group_rank, on an engine with the workload rows); without it nothing is computed or allocated, and every other row
 * is the same either way.  It is independent of sg_set_rank: both may be on, and neither reads the other.  K11 ranks pods: a
 * Deployment of 20 replicas is 20 nodes of its walk, the mass that reaches the workload is split 20 ways, a rollout renames all of
 * them and the answer is a pod.  This stage walks the workload map instead.  There is no new struct and no new constant: the
 * parameters are sg_rank_params (K11's defaults and checks), the rows sg_node_rank, the seeds SG_RANK_SEED_*.  Integer arithmetic
 * only (u64, every intermediate below 2^64), so the result has one correct value.
 * Over the window's group edges j = 0 .. G-1 (sg_window_groups order, G = min(count, max_edges)) and its workload rows v = 0 .. n-1
 * (sg_window_group_nodes order, ascending group key):
 *   w_j     = edges_j + min(score_q32_j >> 16, 65536 * edges_j), a uint64_t, at most 65537 * edges_j: what the group edge carries
 *             of its rows' 1 + q16(score).  A group edge that folds one row has exactly K11's w of that row.  A group edge whose
 *             from_ref or to_ref has no group key (a ref beyond the id spaces; no window has one) carries w_j = 0.  A group edge
 *             inside a workload (from_ref == to_ref) and an alive-only group edge are ordinary edges
 *   W_u     = sum of w_j over the group edges with from_ref == row u's ref (at most 65537 * E rows, as K11)
 *   seed    K11's rule over the workload rows: SG_RANK_SEED_SCORE: a_v = row.score >= seed_min_score ? q16(row.score) : 0;
 *           SG_RANK_SEED_UNIFORM: a_v = 1;  A = sum of a_v; A == 0: the seed falls back to uniform (a_v = 1, A = n)
 *   M = 2^56;  p_v = a_v * floor(M / A);  D = damping_q8;  R_v = (p_v >> 8) * (256 - D);  r_v = p_v
 *   one iteration, `iters` times:
 *           m_u = (r_u >> 8) * D;  t_u = W_u ? floor(m_u / W_u) : 0;
 *           r'_v = R_v + (m_v - t_v * W_v) + sum over the group edges j with to_ref == row v's ref of t_{from_j} * w_j
 *   row v   rank = r_v after the last iteration, ref = the workload row's group ref, share = (float)((double)rank * 2^-56)
 * Invariants (K11's, unchanged): sum r' == sum R + sum m exactly, and sum r <= M; hence t_u * w_j <= m_u < 2^56.
 * Under a map that groups nothing the workload rows are the node rows and every group edge is one row: the rank rows then equal
 * sg_window_rank's of the same window byte for byte (floor(s * 2^32) >> 16 == floor(s * 2^16) for every score).
 * Selection is K11's over these rank rows: key min(rank >> 24, 0xFFFFFFFF), key 0 is not a candidate, share >= min_share, k = 0
 * every candidate in row order, 1 <= k <= SG_SELECT_MAX_K the highest keys descending, ties by row position; the selected rows are
 * byte-identical to sg_window_group_nodes'.
 * State: sg_set_group_rank is SG_ESTATE with the workload rows off (sg_set_group_nodes) or while a flush is open, SG_EINVAL on bad
 * parameters; NULL = off (frees its memory).  Memory is allocated there, never at sg_create, sg_set_groups or sg_set_group_nodes.
 * sg_set_group_nodes(h, 0) and ANY sg_set_groups call switch it off and free it; sg_group_assign does not touch it.  Reads of a
 * window closed while it was off: SG_ESTATE.  Every close path computes it (one call, begin + end, the views, the _top flushes,
 * sg_window_run, the staged sg_window_score), behind K16 and K16's baseline on the window's stream.                              */
int sg_set_group_rank(sg_handle h, const sg_rank_params* p);
/* The rank rows of the last READ window (as sg_window_rank): node_index NULL: every workload row, *n = workload rows; else out[k] =
 * the row of workload row node_index[k] (each < workload rows, else SG_EINVAL), *n = n_index.  min(*n, cap) rows are written.      */
int sg_window_group_rank(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_rank* out, size_t cap, size_t* n);
/* Device sg_node_rank[] of the window sg_window_run closed last (its count is sg_window_group_nodes_buffer's; valid until the slot
 * is reused; read it on that window's stream).                                                                                   */
int sg_window_group_rank_buffer(sg_handle h, void** d_rank);
/* sg_window_rank_top / sg_window_rank_select with "node row" read as "workload row": out [cap] workload rows, rank_out [cap] their
 * rank rows, node_index [cap] their positions (each may be NULL).  k > SG_SELECT_MAX_K: SG_EINVAL.                                */
int sg_window_group_rank_top(sg_handle h, uint32_t k, float min_share, sg_node_out* out, sg_node_rank* rank_out,
                             uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);
int sg_window_group_rank_select(sg_handle h, uint32_t k, float min_share, sg_node_out* d_out, uint32_t* d_index,
                                size_t cap, uint64_t* d_n, void* stream);

/* ---- workload incidents (K18): each window's anomalous group edges grouped into connected components, on the device ------------ *
 * Opt-in (sg_set_group_incidents, on an engine with the workload rows); without it nothing is computed or allocated, and every other
 * row is the same either way.  It is independent of sg_set_incidents: both may be on, and neither reads the other.  K12 groups pods:
 * its trend keys read K8's baseline, which a rollout forgets; its fields are node rows and its culprit K11's; and two pods of one
 * workload failing towards two callees are two incidents.  This stage is K12's definition over the contracted graph, valued by K15
 * and carrying K17's culprit.  There is no new struct and no new constant: the parameters are sg_incident_params (K12's checks), the
 * rows sg_incident_out, "no incident" SG_NO_INCIDENT.
 * Over the window's group edges j = 0 .. G-1 (sg_window_groups order, G = min(count, max_edges)) and its workload rows v = 0 .. n-1
 * (sg_window_group_nodes order, cut at the slot's row capacity):
 *   value_j  `by` = SG_SEL_SCORE: the group edge's score_max (what sg_window_groups_top keys); SG_SEL_LAT_DEV / SG_SEL_ERR_DEV: this
 *            window's sg_window_group_trend row j, .lat_dev / .err_dev.  Any other `by`: SG_EINVAL
 *   red      group edge j is red iff value_j >= min_value (a plain float comparison, NaN never) and both its from_ref and its
 *            to_ref have a workload row at a position < n (a ref without a group key, or whose row was cut at the capacity, makes
 *            the group edge not red).  Alive-only group edges and group edges inside a workload are ordinary group edges
 *   graph    K12's: undirected, on the workload rows, one edge {from, to} per red group edge.  A workload row is in an incident
 *            iff it is an endpoint of a red group edge (a red group edge with from_ref == to_ref makes its row an incident on its
 *            own); the incidents are the connected components of those rows, numbered 0 .. I-1 by ascending first_node
 * Incident i (sg_incident_out):
 *   first_node, nodes    its smallest workload row (an index into sg_window_group_nodes); its workload rows
 *   top_node             the workload row with the largest sg_node_out.score among them (by the order-preserving bits of the
 *                        score, +0.0 above -0.0), ties to the smallest index
 *   edges                its red GROUP EDGES (other group edges between its rows do not count)
 *   count, err, sum_ns,  wrapping u64 sums of those group edges' count, err_count, sum_ns and score_q32: the group edge's fields as
 *   score_q32            they stand, so every row folded into a red group edge counts, whether or not it would be red on its own
 *   value_max, worst_row the largest value_j among its red group edges, +0.0 above -0.0; the smallest GROUP-EDGE INDEX that has it:
 *                        worst_row indexes sg_window_groups, and that group edge's own worst_row leads on to the pod row
 *   culprit_node         with the workload ranking (K17, sg_set_group_rank) on for the window: the workload row with the largest
 *   rank_sum             sg_node_rank.rank among its rows, ties to the smallest index; the wrapping u64 sum of its rows' rank.
 *                        K17 off: SG_NO_INCIDENT and 0.  K11 (sg_set_rank) is never read
 *   reserved             0
 * Every field is an integer sum, an integer max or a max of (order-preserving float bits << 32 | ~index): the result has one
 * correct value.  Under a map that groups nothing the workload rows are the node rows and every group edge is one row: with
 * `by` = SG_SEL_SCORE the incidents then equal sg_window_incidents' of the same window byte for byte, culprit_node and rank_sum
 * too when K11 and K17 run with the same parameters.
 * State: sg_set_group_incidents is SG_ESTATE with the workload rows off (sg_set_group_nodes), while a flush is open, or when `by`
 * is a trend key and the group trend (sg_set_group_trend) is off; SG_EINVAL on bad parameters (struct_size, `by`, a non-zero
 * reserved); NULL = off (frees its memory).  Memory is allocated there, never at sg_create, sg_set_groups or sg_set_group_nodes.
 * sg_set_group_nodes(h, 0) and ANY sg_set_groups call switch it off and free it; sg_set_group_trend(h, NULL) does so only when `by`
 * is a trend key; sg_group_assign, sg_set_group_rank, sg_set_incidents and sg_set_tracks do not touch it, and it touches none of
 * them.  Reads of a window closed while it was off, and while a flush is open: SG_ESTATE.  Every close path computes it (one call,
 * begin + end, the views, the _top flushes, sg_window_run, the staged sg_window_score), behind K15 (a trend key), K16 and its
 * baseline, and K17 on the window's stream.                                                                                    */
int sg_set_group_incidents(sg_handle h, const sg_incident_params* p);
/* The workload incidents of the last READ window (as sg_window_incidents): *n = incidents, min(*n, cap) rows are written.       */
int sg_window_group_incidents(sg_handle h, sg_incident_out* out, size_t cap, size_t* n);
/* The incident number of every workload row of the last READ window, SG_NO_INCIDENT for a row in none (as sg_window_node_incident):
 * node_index NULL: every workload row, *n = workload rows; else out[k] = the number of workload row node_index[k] (each < workload
 * rows, else SG_EINVAL), *n = n_index.  min(*n, cap) values are written.                                                        */
int sg_window_group_node_incident(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
/* Device sg_incident_out[], their count (one uint64_t) and uint32_t[workload rows] (the incident per workload row) of the window
 * sg_window_run closed last (valid until its slot is reused; read them on that window's stream).                                */
int sg_window_group_incidents_buffer(sg_handle h, void** d_incidents, void** d_count, void** d_node_incident);

/* ---- workload tracks (K19): each window's workload incidents followed across windows, on the device --------------------------- *
 * Opt-in (sg_set_group_tracks, on an engine with the workload incidents); without it nothing is launched or allocated, and every
 * other output is byte for byte the same either way.  K13 follows pod incidents: its members are keyed by pod and service node ids,
 * so a rollout, which replaces every pod of a Deployment, makes the incident reappear as new tracks with parent == SG_NO_TRACK.  This
 * stage is the "tracks" section above, steps 1 - 9 word for word, with "incident" read as "workload incident" (K18:
 * sg_window_group_incidents, sg_window_group_node_incident) and "node row" read as "workload row" (K16: sg_window_group_nodes).  There
 * is no new struct and no new constant: the parameters are sg_track_params (K13's checks), the rows sg_incident_track, the table and
 * the ended list sg_track_entry, the counters sg_track_stats, "no track" SG_NO_TRACK, the flags SG_TRACK_*.  The differences:
 *   anchor      a workload row whose ref is a GROUP, KNOWN or LABEL ref; an OBIP ref is no anchor.  The anchor key is K16's group key:
 *               a group's id, max_groups + id for an ungrouped pod or service, max_groups + max_known_nodes + id for a label; the
 *               outbound IPs' keys lie above those and never anchor, and a ref beyond the id spaces has no key.  A workload row has
 *               a pod, a service or a workload at one end, so every workload incident has an anchor
 *   members     kept by that key: max_groups + max_known_nodes + max_labels of them.  A member belongs to the KEY, not to the pods
 *               behind it: nothing migrates a member when sg_group_assign moves a pod from one group to another or out of every
 *               group.  The row then appears under its new key, which has a member of its own or none, and the old key's member
 *               simply ages out after quiet_windows
 *   w           the windows closed since sg_set_group_tracks switched it on (the first: 0)
 *   capacities  the incidents and the ended list of a window are cut at the workload rows' capacity (min(max_groups + node
 *               capacity, 2 x max_edges)); max_tracks 0 = (quiet_windows + 1) * that capacity: nothing is ever cut
 * State: sg_set_group_tracks is SG_ESTATE with the workload incidents off (sg_set_group_incidents) or while a flush is open, SG_EINVAL
 * on bad parameters; NULL = off (frees its memory); (re)enabling starts an empty state at w = 0, next id 0.  Memory is allocated
 * there, never at sg_create or at any other sg_set_group_* call.  EVERY sg_set_group_incidents call, on or off, switches it off and
 * frees it, and so does whatever frees the workload incidents: sg_set_group_nodes(h, 0), any sg_set_groups call,
 * sg_set_group_trend(h, NULL) under a trend key.  It is independent of sg_set_tracks: both may be on in one engine, each with its
 * own members, table, w and ids, and neither reads the other.  Reads of a window closed while it was off, and while a flush is
 * open: SG_ESTATE.  Every close path computes it, behind K18 on the window's stream; with several windows in flight the state
 * updates run in window order.  Under a map that groups nothing the workload rows are the node rows, and with the same parameters
 * and both stages switched on before the same window the rows, ended lists, tables and counters equal K13's byte for byte.         */
int sg_set_group_tracks(sg_handle h, const sg_track_params* p);
/* Row i belongs to workload incident i of the last READ window (as sg_window_incident_tracks).                                  */
int sg_window_group_incident_tracks(sg_handle h, sg_incident_track* out, size_t cap, size_t* n);
/* The ended list of the last READ window (as sg_window_tracks_ended).                                                           */
int sg_window_group_tracks_ended(sg_handle h, sg_track_entry* out, size_t cap, size_t* n);
/* Device sg_incident_track[] (their count is sg_window_group_incidents_buffer's), the ended sg_track_entry[] and their count (one
 * uint64_t) of the window sg_window_run closed last (valid until its slot is reused; read them on that window's stream).        */
int sg_window_group_tracks_buffer(sg_handle h, void** d_tracks, void** d_ended, void** d_ended_count);
/* The live table in id order (as sg_track_entries) and the counters (as sg_track_stats_get); both wait for the updates enqueued
 * so far.                                                                                                                     */
int sg_group_track_entries(sg_handle h, sg_track_entry* out, size_t cap, size_t* n);
int sg_group_track_stats_get(sg_handle h, sg_track_stats* out);

/* ---- workload impact (K22): who depends on each workload incident, and what entered through them, on the device --------------- *
 * Opt-in (sg_set_group_impact, on an engine with the workload incidents); without it nothing is launched or allocated, and every
 * other output is byte for byte the same either way.  Given an incident at `db`: which workloads call it, directly or through
 * others, and how much traffic entered the system through workloads upstream of it?  A capped selection cannot answer that (the
 * callers of an incident are mostly not red), and a host search needs every group edge copied out first.  Workload space only: in
 * pod space a row's source is always a pod, so a Service node has no outgoing row and nothing is more than one hop upstream.
 * There is no new struct: the rows are plain uint64_t / uint32_t arrays.  Over the last closed window's group edges j
 * (sg_window_groups order), its workload rows v (sg_window_group_nodes order), its workload incidents i < I
 * (sg_window_group_incidents) and inc[v] (sg_window_group_node_incident):
 *   covered     incident i is covered iff i < min(I, max_incidents); W = ceil(max_incidents / 64) mask words per workload row
 *   call edge   a group edge with count > 0 whose from_ref and to_ref both have workload rows u != v: "u calls v".  Alive-only
 *               group edges, traffic inside one workload and an endpoint cut at the row capacity never count
 *   d_i(x)      0 if inc[x] == i; otherwise the fewest call edges on a directed path from x to a member of i, infinite without one
 *   exposed     x is exposed to i iff 1 <= d_i(x) <= max_hops;  reach_i = the members of i and its exposed rows
 *   entry row   a workload row at which no call edge arrives
 * Impact row i (SG_IMPACT_WORDS uint64_t words):
 *   EXPOSED     the exposed rows                          DIRECT   the rows with d_i == 1
 *   FAR         hops << 32 | row: the largest d_i among the exposed rows and the smallest row that has it; 0x00000000FFFFFFFF when
 *               nothing is exposed.  hops == max_hops: the search may have been cut
 *   ENTRIES     the entry rows in reach_i                 ENTRY_COUNT, ENTRY_ERR   the wrapping sums of their out_count, out_err
 *   INTO_COUNT, INTO_ERR   the wrapping sums of count and err_count over the call edges with inc[to] == i and inc[from] != i
 * Per workload row v: hops[v] = the smallest d_i(v) over the covered incidents if that is at most max_hops (a member: 0), else
 * SG_NO_HOPS; mask[v][w] bit b is set iff incident 64 w + b is covered and d_i(v) <= max_hops (members included).  Every value is
 * an integer sum or the max of a key: the result has one correct value.  Every close path computes it, behind K18 on the window's
 * stream: 2 max_hops + 4 launches, most of which return at their first load once a round reaches no new row.
 * State: sg_set_group_impact(h, max_incidents, max_hops) — 0, 0 switches it off and frees its memory; on needs
 * 1 <= max_incidents <= SG_IMPACT_MAX_INCIDENTS and 1 <= max_hops <= SG_IMPACT_MAX_HOPS, anything else is SG_EINVAL; SG_ESTATE with
 * the workload incidents off (sg_set_group_incidents) or while a flush is open.  Memory is allocated there, never at sg_create or at
 * any other sg_set_* call.  EVERY sg_set_group_incidents call, on or off, switches it off and frees it, and so does whatever frees
 * the workload incidents (as the workload tracks).  Reads of a window closed while it was off, and while a flush is open: SG_ESTATE. */
#define SG_IMPACT_WORDS          8u
#define SG_IMPACT_MAX_INCIDENTS  1024u
#define SG_IMPACT_MAX_HOPS       64u
#define SG_NO_HOPS               0xFFFFFFFFu
/* word indices of an impact row */
#define SG_IMPACT_EXPOSED     0u
#define SG_IMPACT_DIRECT      1u
#define SG_IMPACT_FAR         2u
#define SG_IMPACT_ENTRIES     3u
#define SG_IMPACT_ENTRY_COUNT 4u
#define SG_IMPACT_ENTRY_ERR   5u
#define SG_IMPACT_INTO_COUNT  6u
#define SG_IMPACT_INTO_ERR    7u
int sg_set_group_impact(sg_handle h, uint32_t max_incidents, uint32_t max_hops);
/* The impact rows of the last READ window: *n = min(I, max_incidents) rows, min(*n, cap_rows) rows of SG_IMPACT_WORDS words each
 * are written; row i belongs to sg_window_group_incidents' row i.                                                              */
int sg_window_group_impact(sg_handle h, uint64_t* out, size_t cap_rows, size_t* n);
/* hops of every workload row of the last READ window (as sg_window_group_node_incident): node_index NULL: every workload row,
 * *n = workload rows; else out[k] = hops of workload row node_index[k] (each < workload rows, else SG_EINVAL), *n = n_index.
 * min(*n, cap) values are written.                                                                                             */
int sg_window_group_node_hops(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
/* The mask rows of the last READ window: *n = workload rows, *words = W, min(*n, cap_rows) rows of W words each are written.     */
int sg_window_group_impact_mask(sg_handle h, uint64_t* out, size_t cap_rows, size_t* n, uint32_t* words);
/* Device impact rows (uint64_t[max_incidents][SG_IMPACT_WORDS]), the covered count (one uint64_t), uint32_t hops[workload rows]
 * and the mask rows (uint64_t[workload rows][W]) of the window sg_window_run closed last (valid until its slot is reused; read
 * them on that window's stream).                                                                                               */
int sg_window_group_impact_buffer(sg_handle h, void** d_impact, void** d_count, void** d_hops, void** d_mask);

/* ---- latency percentiles (K20): histograms and percentiles per node row, group edge and workload row, on the device ----------- *
 * Opt-in (sg_set_quantiles, on an engine created with SG_CFG_EDGE_HISTOGRAM); without it nothing is launched or allocated, and
 * every other output is byte for byte the same either way.  Percentiles do not average: a node's, a group edge's or a workload's
 * p99 follows from the MERGED histogram of its rows only.  Let H_r[16] be the bins of row r as sg_window_hist returns them.  Three
 * spaces, each with histograms of uint64_t bins (a sum of up to 2^32 uint32_t bins cannot wrap):
 *   nodes        (SG_Q_NODES; needs sg_set_nodes) for node row x of sg_window_nodes: out[b] = sum of H_r[b] over the rows with
 *                from_ref == x's ref, in[b] over the rows with to_ref == x's ref.  A self-loop counts on both sides, as in K9
 *   group edges  (SG_Q_GROUPS; needs sg_set_groups) for group edge g of sg_window_groups: B[b] = sum of H_r[b] over the rows of its
 *                run, perm[first .. first + edges)
 *   workloads    (SG_Q_GROUP_NODES; needs sg_set_group_nodes) for workload row x of sg_window_group_nodes: the nodes' definition
 *                with every ref replaced by its group ref; equally, the sum over the group edges on that side
 * The quantile Q(B, max_ns, qm) of a histogram B at qm per-mille (1 .. 1000):
 *   total = sum of B (every bin of a row's histogram counts one request of the row, so total equals the entity's count /
 *   out_count / in_count; the definition is the sum of the bins).  total == 0: Q = 0.  Otherwise
 *   rank = max(1, (total / 1000) * qm + ceil((total % 1000) * qm / 1000)) — ceil(total * qm / 1000) without overflow;
 *   b = the first bin whose cumulative count reaches rank; edge_ns = (b == 15) ? max_ns : 2^(17 + b), then capped at max_ns;
 *   Q = edge_ns / 1000 (floor), saturated to uint32_t.
 * max_ns is the entity's own: sg_group_edge.max_ns, sg_node_out.out_max_ns / in_max_ns of the side.  At qm = 500 and 990 this is
 * the rule of a row's p50_us / p99_us: a group edge of one row has that row's percentiles.  Every value is an integer sum or follows
 * from one: the result has one correct value.  Every close path computes it (one call, begin + end, the views, the _top / _top_by
 * flushes, sg_window_run, the staged sg_window_score), behind K9 / K14 / K16 on the window's stream.
 * State: sg_set_quantiles(h, spaces, permille, n_q) — spaces == 0 switches the stage off and frees its memory; n_q == 0 means
 * {500, 990}.  SG_EINVAL for unknown bits, n_q > SG_Q_MAX, a per-mille outside 1 .. 1000, or an engine with world > 1; SG_ESTATE on
 * an engine without SG_CFG_EDGE_HISTOGRAM, for a space whose base stage is off, or while a flush is open.  Memory is allocated
 * there, never at sg_create: the group edges' table alone is 128 bytes x max_edges per window slot, which is why each space is
 * asked for by its own bit.  Every call replaces the previous setting.  Switching a base stage off frees this stage's space with
 * it: sg_set_nodes(h, 0) the nodes', any sg_set_groups call the group edges' and the workloads', sg_set_group_nodes(h, 0) the
 * workloads'.  Reads of a window closed while the space was off, and while a flush is open: SG_ESTATE.                            */
#define SG_Q_NODES        1u
#define SG_Q_GROUPS       2u
#define SG_Q_GROUP_NODES  4u
#define SG_Q_MAX          8u    /* quantiles per entity and side at most                          */
int sg_set_quantiles(sg_handle h, uint32_t spaces, const uint32_t* permille, size_t n_q);
/* The histograms and the quantiles of the last READ window (as sg_window_node_trend): index NULL: every entity of the space, *n =
 * their count; else out[k] = the entry of entity index[k] (each < the count, else SG_EINVAL), gathered on the device, *n = n_index.
 * cap counts entities; min(*n, cap) entries are written.  An entry of sg_window_node_hist / sg_window_group_node_hist is [2][16]
 * uint64_t (out side, then in side), of sg_window_group_hist [16]; of sg_window_node_quantiles / sg_window_group_node_quantiles
 * [2][n_q] uint32_t microseconds, of sg_window_group_quantiles [n_q], in the order of sg_set_quantiles' permille.                */
int sg_window_node_hist(sg_handle h, const uint32_t* node_index, size_t n_index, uint64_t* out, size_t cap, size_t* n);
int sg_window_node_quantiles(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out_us, size_t cap, size_t* n);
int sg_window_group_hist(sg_handle h, const uint32_t* group_index, size_t n_index, uint64_t* out, size_t cap, size_t* n);
int sg_window_group_quantiles(sg_handle h, const uint32_t* group_index, size_t n_index, uint32_t* out_us, size_t cap, size_t* n);
int sg_window_group_node_hist(sg_handle h, const uint32_t* node_index, size_t n_index, uint64_t* out, size_t cap, size_t* n);
int sg_window_group_node_quantiles(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out_us, size_t cap, size_t* n);
/* Device tables of space `space` (one SG_Q_* bit) of the window sg_window_run closed last (valid until its slot is reused; read
 * them on that window's stream): the histograms as the reads above lay them out, and the quantiles with SG_Q_MAX uint32_t per
 * entity and side, the first n_q of them set.  The entity count is the space's own (sg_window_nodes_buffer, ...).               */
int sg_window_quantiles_buffer(sg_handle h, uint32_t space, void** d_hist, void** d_quantiles);

/* ---- tail baselines (K21): each entity's tracked quantile against its own past, on the device -------------------------------------- *
 * Opt-in (sg_set_quantile_trend, on an engine on which sg_set_quantiles has switched the requested spaces on); without it nothing
 * is launched or allocated, and every other output is byte for byte the same either way.  For each requested K20 space there is
 * one baseline with a trend-window counter of its own.  Its keys and its sample order are those of the mean baseline of that space:
 *   SG_Q_NODES        sample 2 * node + side, side 0 = in, 1 = out; key (nk, side), the node baselines'; rows sg_node_trend
 *   SG_Q_GROUPS       sample = group edge j; key (wk(from_ref), wk(to_ref)), the group baselines'; rows sg_edge_trend
 *   SG_Q_GROUP_NODES  sample 2 * row + side; key (wk(ref), side), the workload baselines'; rows sg_node_trend
 * The sample of an entity side with count c > 0 (c the count the mean baseline of the space reads: in_count / out_count of the node
 * row, count of the group edge): x_lat = 1000.0 * Q, Q the uint32_t microsecond value K20 wrote for the tracked per-mille of that
 * entity and side in this window — exact in fp64 (Q < 2^32, x_lat < 2^52); x_err is the space's own error sample, unchanged: the
 * long division floor(err * 2^20 / c).  A side with c == 0 neither creates nor refreshes an entry.
 * Side order: K20's tables hold a node's sides as [0] = out, [1] = in, the node baselines' samples are side 0 = in, 1 = out: the
 * sample of side s reads K20 side 1 - s.
 * Entry update, expiry (ttl), the capacity cut, the statistics and the row rule are the trend's (sg_set_trend) word for word: rows
 * are scored from the entry as it stood before the window's update, zero below warmup or when c == 0, base_mean_us = (float)
 * (lat_mean / 1000).  In a row lat_dev is the deviation of the tracked quantile, err_dev the error-rate deviation as in the mean
 * baseline, base_mean_us the baseline of the quantile.  max_entries == 0 resolves to the default of the mean baseline of the
 * space: 4 x the node rows (workload rows) a window can have for the two node-shaped spaces, 2 x max_edges for the group edges.
 * Every close path computes it, behind K20 of the same window on the window's stream; with several windows in flight the state
 * updates run in window order.
 * State: sg_set_quantile_trend(h, spaces, permille, p) — spaces == 0 or p == NULL switches the stage off and frees it; every call
 * replaces the previous setting and starts empty baselines; one sg_trend_params serves all requested spaces.  SG_EINVAL for
 * unknown space bits, bad parameters (sg_set_trend's checks) or a permille that is not among the per-mille sg_set_quantiles was
 * last given (the tracked quantile's index is its position there); SG_ESTATE for a space K20 has not on, or while a flush is
 * open.  Memory is allocated there, never at sg_create.  ANY sg_set_quantiles call that is not refused switches this stage
 * off and frees it (the quantile's index may have moved), and whatever frees a K20 space frees this stage's baseline of that space
 * with it: sg_set_nodes(h, 0), any sg_set_groups call, sg_set_group_nodes(h, 0).  It does not touch the mean baselines, nor they it. */
int sg_set_quantile_trend(sg_handle h, uint32_t spaces, uint32_t permille, const sg_trend_params* p);
/* The tail rows of the last READ window, the buffer, the entries and the statistics: exactly sg_window_node_trend,
 * sg_window_node_trend_buffer, sg_node_trend_entries and sg_node_trend_stats_get over the tail baseline of the space (SG_ESTATE for
 * a window closed while it was off).  `space` is exactly one SG_Q_* bit, else SG_EINVAL.                                           */
int sg_window_node_quantile_trend(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
int sg_window_group_quantile_trend(sg_handle h, const uint32_t* group_index, size_t n_index, sg_edge_trend* out, size_t cap, size_t* n);
int sg_window_group_node_quantile_trend(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
int sg_window_quantile_trend_buffer(sg_handle h, uint32_t space, void** d_trend);
int sg_quantile_trend_entries(sg_handle h, uint32_t space, sg_trend_entry* out, size_t cap, size_t* n);
int sg_quantile_trend_stats_get(sg_handle h, uint32_t space, sg_trend_stats* out);
/* sg_window_nodes_top / sg_window_groups_top / sg_window_group_nodes_top with the TAIL rows as the trend source: the same `by`
 * keys (SG_NSEL_* for the node-shaped spaces, SG_SEL_* for the group edges), the same selection, row bytes and index outputs.
 * SG_ESTATE when the space's tail baseline is off or the window was closed while it was.                                          */
int sg_window_nodes_top_tail(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);
int sg_window_groups_top_tail(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_group_edge* out, uint32_t* group_index, size_t cap, size_t* n_selected, size_t* n_groups);
int sg_window_group_nodes_top_tail(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);

/* ---- traffic baselines (K23): each entity's request rate and load against its own past, on the device ------------------------------ *
 * Opt-in (sg_set_traffic_trend); without it nothing is launched or allocated, and every other output is byte for byte the same
 * either way.  Every other baseline judges a window by latency or error ratio; this one by HOW MUCH traffic an entity carried: a
 * partial drop (an upstream failure cuts off most of the requests, the ones that still arrive are fast and succeed) or a surge (a
 * retry storm, a new client) shows here while lat_dev, err_dev and the scores stay calm.
 * Four bits select the spaces; each requested space gets one baseline with a trend-window counter of its own, with the keys, the
 * sample order and the row type of the MEAN baseline of that space:
 *   SG_T_EDGES        sample = row j of the window; key (from_key, to_key), the trend's (sg_set_trend); rows sg_edge_trend
 *   SG_T_NODES        sample 2 * node + side, side 0 = in, 1 = out; key (nk, side), the node baselines'; rows sg_node_trend
 *   SG_T_GROUPS       sample = group edge j; key (wk(from_ref), wk(to_ref)), the group baselines'; rows sg_edge_trend
 *   SG_T_GROUP_NODES  sample 2 * row + side; key (wk(ref), side), the workload baselines'; rows sg_node_trend
 * A space needs only its rows: SG_T_NODES needs sg_set_nodes, SG_T_GROUPS sg_set_groups, SG_T_GROUP_NODES sg_set_group_nodes
 * (SG_ESTATE otherwise), SG_T_EDGES nothing.  The stage needs neither the mean baselines nor K20 and does not touch them, nor
 * they it.  Whatever frees a space's rows frees this stage's baseline of that space with it: sg_set_nodes(h, 0), any
 * sg_set_groups call, sg_set_group_nodes(h, 0).
 * Samples.  An entity side has the count c the mean baseline of the space reads (count of the row or group edge, in_count /
 * out_count of the node or workload row) and its sum_ns.  With c > 0 its two samples are exact integers in fp64:
 *   x_rate = 1000.0 * min(c, 2^42)       so that base_mean_us = (float)(mean / 1000) reads as REQUESTS PER WINDOW
 *   x_load = (double) min(sum_ns, 2^52)  the side's busy time, requests x latency: by Little's law the concurrency the callee
 *                                        carried over the window
 * x_rate feeds the lat_* half of the entry (sg_trend_entry.lat_mean / lat_dev) and of the row, x_load the err_* half.  In a row
 *   lat_dev       is the RATE deviation, (x_rate - mean) / max(dev, 1000.0 * rate_floor)
 *   err_dev       is the LOAD deviation, (x_load - mean) / max(dev, load_floor_ns)
 *   base_mean_us  is the baseline RATE in requests per window
 *   windows_seen  (in_seen / out_seen) keeps its name and meaning
 * and for the node-shaped rows in_* / out_* are the two sides as in sg_node_trend.  A drop is a negative deviation.
 * Absent entities.  A side with c == 0, or an entity without a row in the window, neither creates, refreshes nor scores an entry,
 * as in every other baseline.  COMPLETE silence stays the business of the vanished lists (sg_set_vanished, sg_set_group_vanished):
 * this stage is about partial drops and surges.  Windows are ASSUMED TO BE OF EQUAL LENGTH: the samples are per window, not per
 * second, and a host that closes windows of varying length sees that as a change of rate.
 * Entry update, expiry (ttl), the capacity cut, the statistics and the row rule are the trend's (sg_set_trend) word for word: rows
 * are scored from the entry as it stood before the window's update, zero below warmup or when c == 0.
 * Every close path computes it, behind the space's rows of the same window on the window's stream; with several windows in flight
 * the state updates run in window order.                                                                                          */
#define SG_T_EDGES        1u
#define SG_T_NODES        2u
#define SG_T_GROUPS       4u
#define SG_T_GROUP_NODES  8u
typedef struct sg_traffic_params {
    uint32_t struct_size;       /* sizeof(sg_traffic_params)                                                                */
    uint32_t shift;             /* alpha = 2^-shift, 1..10 (0 = 4)                                                           */
    uint32_t warmup;            /* windows an entry must have seen before its rows report deviations (0 = 4)                 */
    uint32_t ttl;               /* windows an entry survives without a sample (0 = 64)                                       */
    uint64_t max_entries;       /* capacity of each space's baseline, at most 2^31 (0 = the default of the mean baseline of
                                 * that space: 2 x max_edges for the two edge-shaped spaces, 4 x the rows a window can have for
                                 * the two node-shaped ones)                                                                 */
    uint64_t load_floor_ns;     /* load deviation floor in ns of busy time, at most 2^52 (0 = 1 000 000)                     */
    uint32_t rate_floor;        /* rate deviation floor in requests (0 = 8)                                                  */
    uint32_t reserved;          /* 0                                                                                         */
} sg_traffic_params;            /* 40 bytes, no padding */
/* spaces == 0 or p == NULL switches the stage off and frees it; every call replaces the previous setting and starts empty
 * baselines; one sg_traffic_params serves all requested spaces.  SG_EINVAL for unknown space bits or bad parameters; SG_ESTATE for
 * a space whose rows are off, or while a flush is open.  Memory is allocated here, never at sg_create.                           */
int sg_set_traffic_trend(sg_handle h, uint32_t spaces, const sg_traffic_params* p);
/* The traffic rows of the last READ window, one call per space: exactly sg_window_trend, sg_window_node_trend,
 * sg_window_group_trend and sg_window_group_node_trend over the traffic baseline of the space.                                   */
int sg_window_traffic(sg_handle h, const uint32_t* row_index, size_t n_index, sg_edge_trend* out, size_t cap, size_t* n);
int sg_window_node_traffic(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
int sg_window_group_traffic(sg_handle h, const uint32_t* group_index, size_t n_index, sg_edge_trend* out, size_t cap, size_t* n);
int sg_window_group_node_traffic(sg_handle h, const uint32_t* node_index, size_t n_index, sg_node_trend* out, size_t cap, size_t* n);
/* The device rows of one space of the window sg_window_run closed last (as sg_window_trend_buffer and its twins), the baseline in
 * key order and its statistics (as sg_trend_entries / sg_trend_stats_get).  `space` is exactly one SG_T_* bit, else SG_EINVAL.   */
int sg_window_traffic_buffer(sg_handle h, uint32_t space, void** d_rows);
int sg_traffic_trend_entries(sg_handle h, uint32_t space, sg_trend_entry* out, size_t cap, size_t* n);
int sg_traffic_trend_stats_get(sg_handle h, uint32_t space, sg_trend_stats* out);
/* Selections over the traffic rows of the last READ window, with the argument lists, the row bytes and the index outputs of their
 * _top_tail twins.  `by` is one of the four keys below — the SIGNED value is what is ranked, so a drop is selected by its size —
 * and on the two node-shaped spaces it is ORed with exactly one of SG_TSEL_IN / SG_TSEL_OUT (the side; on the group edges with
 * neither); anything else is SG_EINVAL.  min_value and the tie rule (by row position, -0.0 == +0.0) are the other selections',
 * applied to the signed value: SG_TSEL_DROP with min_value 3 selects the rows whose rate fell by more than three deviations.
 * There is no "new" key: SG_NSEL_NEW / SG_SEL_NEW over the mean baselines answer that.  The pod-edge space (SG_T_EDGES) has no
 * _top_traffic: its host form would be a flush; read its rows with sg_window_traffic at the indices another selection gave.
 * SG_ESTATE when the space's traffic baseline is off or the window was closed while it was.                                      */
#define SG_TSEL_SURGE      0u   /* +rate deviation */
#define SG_TSEL_DROP       1u   /* -rate deviation */
#define SG_TSEL_LOAD_UP    2u   /* +load deviation */
#define SG_TSEL_LOAD_DOWN  3u   /* -load deviation */
#define SG_TSEL_IN         4u   /* the in side of a node or workload row: the calls it receives */
#define SG_TSEL_OUT        8u   /* the out side: the calls it makes */
int sg_window_nodes_top_traffic(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);
int sg_window_groups_top_traffic(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_group_edge* out, uint32_t* group_index, size_t cap, size_t* n_selected, size_t* n_groups);
int sg_window_group_nodes_top_traffic(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* node_index, size_t cap, size_t* n_selected, size_t* n_nodes);

/* ---- SLO burn rates (K24): is each service and workload meeting its objective, and how fast does it burn its budget --------------- *
 * Opt-in (sg_set_slo); without it nothing is launched or allocated, and every other output is byte for byte the same either way.
 * Every baseline asks whether a window is unusual against the entity's own past.  This stage asks the on-call question: an
 * ABSOLUTE objective ("99.9 % of requests succeed", "99 % are faster than 134 ms"), the bad fraction over a short and a long span
 * of windows as EXACT sums, each divided by the error budget: the multi-window, multi-burn-rate alert.  A service that has
 * always served 2 % errors is calm in every baseline and burning here.
 * Spaces.  The two node-shaped K20 spaces, named by their SG_Q_* bits: SG_Q_NODES (the node rows of sg_window_nodes) and
 * SG_Q_GROUP_NODES (the workload rows of sg_window_group_nodes).  A space needs K20 on for it (sg_set_quantiles), SG_ESTATE
 * otherwise; whatever frees a space's K20 tables frees this stage's state of that space first: any sg_set_quantiles call,
 * sg_set_nodes(h, 0), any sg_set_groups call, sg_set_group_nodes(h, 0).  Pod edges and group edges have no SLO state.
 * Key.  A row is TRACKED when its ref is KNOWN or LABEL (node space) or GROUP, KNOWN or LABEL (workload space); its key is
 *   node space       KNOWN id v -> v, LABEL v -> max_known_nodes + v                      keys = max_known_nodes + max_labels
 *   workload space   GROUP g -> g, KNOWN v -> max_groups + v, LABEL v -> max_groups + max_known_nodes + v   (K16's group key)
 * Rows with an OBIP ref are untracked: their id is a rank in the window's outbound-IP list and changes from window to window (the
 * anchor rule of the workload tracks).  State belongs to the key: sg_group_assign migrates nothing — a pod that joins a workload
 * starts to count under the workload's key, and what it counted under its own stays there until it leaves the spans.
 * Sample.  Per side of a tracked row the window's sample is (total, err, slow): total and err the side's request and error counts
 * of the row (in_count / in_err, out_count / out_err), slow the sum of bins latency_bin + 1 .. 15 of the side's K20 histogram —
 * the requests with duration_ns >= 2^(17 + latency_bin), the lower edge of bin latency_bin + 1.  A key without a row in a window
 * samples zeros on both sides; its old windows still leave the spans on time.
 * Sums.  Per key and side T_S, E_S, W_S — total, err, slow summed over the last S windows — and T_L, E_L, W_L over the last L, all
 * exact uint64_t sums; the closing window is in both spans, and before S (L) windows have closed since sg_set_slo a span covers
 * what exists.  Windows are assumed to be of equal length.
 * Burn rates.  Four per side (err or slow, short or long span), from bad = min(E or W, T) and total = T of the span:
 *   r        = floor(bad * 2^20 / total), 0 when total == 0          (<= 2^20)
 *   burn_q10 = floor(r * 10^6 / (budget_ppm * 1024))                 (<= 1 024 000 000: a uint32_t)
 * in 1/1024 of "exactly on budget": 1024 burns the budget exactly as fast as the objective allows, 14 746 is the 14.4 x of a
 * page.  budget_ppm = 10^6 - target_ppm.  A kind on a side is BURNING when its short burn and its long burn are both >=
 * min_burn_q10 and T_L >= min_requests.
 * Objectives.  sg_slo_params holds the defaults; sg_slo_assign sets an objective WORD per key:
 *   bits 31..28 latency_bin (0 .. 14) | bits 23..12 latency budget code | bits 11..0 error budget code, bits 27..24 zero
 *   a budget code is exp << 10 | mant: budget_ppm = mant * 10^exp with mant 1 .. 1000, exp 0 .. 3, budget_ppm <= 999 999 — three
 *   significant digits of budget from 1 ppm up (two targets of 20 bits each do not fit a word beside the bin)
 * (SG_SLO_OBJECTIVE builds one).  The word 0 means "the defaults of sg_slo_params"; a valid word is never 0.  A row reports the
 * word it was judged by.  Changing an objective does not rewrite history: the sums are counts, and the slow count of a past
 * window was taken under the latency_bin in force then.
 * Row (SG_SLO_WORDS uint64_t words an entity, row k for row k of the space's node rows):
 *   words 0 .. 7 the in side, 8 .. 15 the out side (sg_node_trend's order); within a side
 *     0 .. 5  T_S, E_S, W_S, T_L, E_L, W_L
 *     6       burn_err_short | (uint64_t) burn_err_long << 32
 *     7       burn_slow_short | (uint64_t) burn_slow_long << 32
 *   word 16   flags | (uint64_t) objective word << 32
 *   word 17   windows the short span covers | (uint64_t) windows the long span covers << 32
 * An untracked row is all zero except SG_SLO_UNTRACKED.
 * Every close path computes it, behind K20 of the same space and window on the window's stream; with several windows in flight
 * the state updates run in window order.  An engine with world > 1 has no K20 and so no SLO stage.                                */
#define SG_SLO_WORDS            18u
#define SG_SLO_MAX_WINDOWS      64u
#define SG_SLO_UNTRACKED        1u    /* flags of word 16 */
#define SG_SLO_ERR_BURNING_IN   2u
#define SG_SLO_SLOW_BURNING_IN  4u
#define SG_SLO_ERR_BURNING_OUT  8u
#define SG_SLO_SLOW_BURNING_OUT 16u
#define SG_SLO_BUDGET_CODE(mant, exp)  (((uint32_t)(exp) << 10) | (uint32_t)(mant))
#define SG_SLO_OBJECTIVE(latency_bin, lat_mant, lat_exp, err_mant, err_exp) \
    (((uint32_t)(latency_bin) << 28) | (SG_SLO_BUDGET_CODE(lat_mant, lat_exp) << 12) | SG_SLO_BUDGET_CODE(err_mant, err_exp))
typedef struct sg_slo_params {
    uint32_t struct_size;        /* sizeof(sg_slo_params)                                                                    */
    uint32_t latency_bin;        /* 0 .. 14: a request is slow when its latency bin is above this value                      */
    uint32_t latency_target_ppm; /* 1 .. 999 999: the default latency objective; its budget is 10^6 - target                 */
    uint32_t error_target_ppm;   /* 1 .. 999 999: the default error objective                                                */
    uint32_t short_windows;      /* S, 1 <= S <= L                                                                           */
    uint32_t long_windows;       /* L, S <= L <= SG_SLO_MAX_WINDOWS: the ring is L x keys x 48 bytes, the caller's choice    */
    uint32_t min_burn_q10;       /* the burn threshold, in 1/1024 of "exactly on budget"                                     */
    uint32_t reserved;           /* 0                                                                                        */
    uint64_t min_requests;       /* a side burns, and is selected, only with T_L >= min_requests                             */
} sg_slo_params;                 /* 40 bytes, no padding */
typedef struct sg_slo_stats {
    uint64_t windows;            /* windows closed since sg_set_slo                                                          */
    uint64_t keys_active;        /* tracked keys with a non-zero T_L on either side                                          */
    uint64_t sides_burning;      /* sides of the last window's rows with a burning kind                                      */
    uint64_t keys;               /* the key space of the stage's state                                                       */
} sg_slo_stats;
/* spaces == 0 or p == NULL switches the stage off and frees it; every call replaces the previous setting and starts empty state
 * (sums, ring, objectives).  spaces: SG_Q_NODES | SG_Q_GROUP_NODES.  SG_EINVAL for other bits, bad parameters or more than 2^21
 * keys; SG_ESTATE for a space K20 has not on, or while a flush is open: such a call leaves the stage as it was.  Memory is
 * allocated here, never at sg_create; a failed allocation (SG_ENOMEM) leaves the stage off.                                      */
int sg_set_slo(sg_handle h, uint32_t spaces, const sg_slo_params* p);
/* Objective words per key of one space (exactly one SG_Q_* bit): refs[i] is a KNOWN or LABEL ref (and a GROUP ref in the workload
 * space) below the engine's id spaces, objectives[i] a valid word or 0; anything else is SG_EINVAL before any word is set.  It
 * waits for the updates enqueued so far and takes effect with the next window closed.                                            */
int sg_slo_assign(sg_handle h, uint32_t space, const uint32_t* refs, const uint32_t* objectives, size_t n);
/* The SLO rows of the last READ window, with the shape of sg_window_group_node_hops: index NULL: every row of the space, *n = their
 * count; else out[k] = the row of entity index[k] (each < the count, else SG_EINVAL), *n = n_index.  cap counts rows of
 * SG_SLO_WORDS words; min(*n, cap) rows are written.                                                                             */
int sg_window_node_slo(sg_handle h, const uint32_t* node_index, size_t n_index, uint64_t* out, size_t cap, size_t* n);
int sg_window_group_node_slo(sg_handle h, const uint32_t* node_index, size_t n_index, uint64_t* out, size_t cap, size_t* n);
/* The device rows (uint64_t[rows][SG_SLO_WORDS]) of one space of the window sg_window_run closed last.                            */
int sg_window_slo_buffer(sg_handle h, uint32_t space, void** d_rows);
/* The state of one space: for each key with a non-zero T_L on either side one entry of SG_SLO_ENTRY_WORDS words — the key, the
 * twelve sums in row order (in: T_S .. W_L, out: T_S .. W_L), the objective word — ascending by key.  *n = their count,
 * min(*n, cap) entries are written.  It waits for the updates enqueued so far, as sg_slo_stats_get does.                          */
#define SG_SLO_ENTRY_WORDS 14u
int sg_slo_entries(sg_handle h, uint32_t space, uint64_t* out, size_t cap, size_t* n);
int sg_slo_stats_get(sg_handle h, uint32_t space, sg_slo_stats* out);
/* Selections over the SLO rows of the last READ window: `by` is SG_SLOSEL_ERR or SG_SLOSEL_SLOW ORed with exactly one of
 * SG_SLOSEL_IN / SG_SLOSEL_OUT, else SG_EINVAL.  A row's value is min(short burn, long burn) of that kind and side, 0 when the row
 * is untracked or T_L < min_requests; the k largest values >= min_value_q10 are selected (k = 0: every such row), ties by row
 * position, rows and indices as sg_window_nodes_top gives them.  "The 20 workloads burning their error budget fastest" is
 * sg_window_group_nodes_top_slo(h, SG_SLOSEL_ERR | SG_SLOSEL_IN, 20, 1024, ...).                                                   */
#define SG_SLOSEL_ERR   0u
#define SG_SLOSEL_SLOW  1u
#define SG_SLOSEL_IN    2u      /* the in side: the calls the entity receives */
#define SG_SLOSEL_OUT   4u      /* the out side: the calls it makes */
int sg_window_nodes_top_slo(sg_handle h, uint32_t by, uint32_t k, uint32_t min_value_q10, sg_node_out* out, uint32_t* index, size_t cap, size_t* n_selected, size_t* n_rows);
int sg_window_group_nodes_top_slo(sg_handle h, uint32_t by, uint32_t k, uint32_t min_value_q10, sg_node_out* out, uint32_t* index, size_t cap, size_t* n_selected, size_t* n_rows);

/* ---- replica outliers (K25): each pod against the other pods of its workload ---------------------------------------------------- *
 * Opt-in (sg_set_replicas); without it nothing is launched or allocated, and every other output is byte for byte the same either
 * way.  Every baseline judges an entity against its own past and the SLO stage against an absolute objective; this stage judges a
 * pod against its SIBLINGS: is `checkout` red, or one replica of it (a bad node, a poisoned connection pool, three times its share
 * of the load)?  The stage is stateless: a window's rows depend on that window alone, and integer arithmetic gives them one value.
 * Members.  Over the closed window's node rows v (sg_window_nodes order) and workload rows w (sg_window_group_nodes order).  Node
 * row v is a MEMBER of workload row w when its ref is KNOWN with id, the device kind[id] is SG_NODE_POD, group[id] = g !=
 * SG_NO_GROUP under the map the window was contracted under, and w is the workload row whose ref is SG_REF_GROUP | g.  Services
 * are never members, not even a Service that service binding has put into the group: its in side is the whole workload's traffic,
 * not a replica's.  LABEL, OBIP and ungrouped nodes are never members.
 * Member sums, per workload row and side s (in or out, sg_node_trend's order), exact uint64_t, T wrapping:
 *   R = members with count_s > 0      C = sum count_s      E = sum err_s      T = sum sum_ns_s
 *   with tails on, H[b] = sum of bin b of the members' K20 node histograms of that side
 * Judged.  Side s of member v with (c, e, S, h[16]) is JUDGED when c >= min_requests, C - c >= min_requests and R >=
 * min_replicas.  The peers are the leave-one-out remainder (C - c, E - e, T - S, H - h); T - S wraps.  For a judged side
 *   x_err(e, c)     = floor(min(e, c) * 2^20 / c)                        (K10's sample rule, by long division)
 *   err_excess_q20  = (int32) x_err(e, c) - (int32) x_err(E - e, C - c)
 *   mean(S, c)      = min(floor(S / c), 2^52)                            (K10's x_lat)
 *   lat_ratio_q10   = min(floor(mean(S, c) * 1024 / max(mean(T - S, C - c), 1)), 2^32 - 1)
 *   share_q10       = min(floor(min(c, 2^53) * 1024 / max(floor(C / R), 1)), 2^32 - 1)      (1024 is exactly the fair share)
 *   tails, only when tail_permille != 0: qbin(h) is the first bin whose cumulative count reaches K20's rank
 *   max(1, ceil(total * permille / 1000)), bin 15 when none does and 0 for total == 0; bins are compared, so no max_ns cap applies
 *   tail_pod = qbin(h), tail_peers = qbin(H - h), tail_excess = tail_pod - tail_peers in octaves
 * A side that is not judged has all of these 0.
 * Example.  Four member pods each received 100 requests; pod A has 10 errors and a 4 000 000 ns mean, the others 1 error each and
 * a 1 000 000 ns mean.  With min_requests 20 and min_replicas 3, A's in side: x_err = 104857, the peers' floor(3 * 2^20 / 300) =
 * 10485, err_excess_q20 = 94372; lat_ratio_q10 = 4096; share_q10 = 1024.
 * Flags.  SG_REPL_MEMBER; per side SG_REPL_JUDGED_*, SG_REPL_ERR_* when err_excess_q20 >= min_err_excess_q20, SG_REPL_LAT_* when
 * lat_ratio_q10 >= min_lat_ratio_q10, SG_REPL_TAIL_* when tails are on and tail_excess >= min_tail_bins.  A side that carries any
 * of ERR, LAT or TAIL is an OUTLIER side.
 * Pod row k (SG_REPLICA_WORDS uint32_t words, for node row k):
 *   word 0        the workload row index, 0xFFFFFFFF for a non-member
 *   word 1        flags
 *   words 2 .. 6  the in side: err_excess_q20 (two's complement), lat_ratio_q10, share_q10, tail_pod | tail_peers << 8, R
 *   words 7 .. 11 the out side, the same
 * A non-member row is 0xFFFFFFFF followed by zeros.
 * Workload row k (SG_REPLICA_GROUP_WORDS words, for workload row k), four words a side, the in side first:
 *   R, judged members, outlier members, the smallest node-row index among the outlier members (0xFFFFFFFF: none)
 * Every close path computes it on the window's stream, behind K16 (and behind K20's node space when tails are on).  An engine
 * with world > 1 has no node rollup and so no replica stage.                                                                      */
#define SG_REPLICA_WORDS        12u
#define SG_REPLICA_GROUP_WORDS  8u
#define SG_REPL_MEMBER      1u      /* flags of word 1 */
#define SG_REPL_JUDGED_IN   2u
#define SG_REPL_ERR_IN      4u
#define SG_REPL_LAT_IN      8u
#define SG_REPL_TAIL_IN     16u
#define SG_REPL_JUDGED_OUT  32u     /* the in side's flags << 4 */
#define SG_REPL_ERR_OUT     64u
#define SG_REPL_LAT_OUT     128u
#define SG_REPL_TAIL_OUT    256u
typedef struct sg_replica_params {
    uint32_t struct_size;        /* sizeof(sg_replica_params)                                                                */
    uint32_t min_replicas;       /* a side is judged with R >= min_replicas; at least 2, 0 = 3                               */
    uint64_t min_requests;       /* ... and with c and C - c >= min_requests; 0 = 20                                         */
    uint32_t min_err_excess_q20; /* 0 = 20972 (two points), at most 2^20                                                     */
    uint32_t min_lat_ratio_q10;  /* 0 = 2048 (twice the peers' mean)                                                         */
    uint32_t tail_permille;      /* 0 = no tails, else 1 .. 999: needs K20's SG_Q_NODES space                                */
    uint32_t min_tail_bins;      /* 0 = 2, at most 15                                                                        */
    uint32_t reserved[2];        /* 0                                                                                        */
} sg_replica_params;             /* 40 bytes, no padding */
/* p == NULL switches the stage off and frees it; every call replaces the previous setting.  SG_EINVAL for bad parameters and on an
 * engine with world > 1; SG_ESTATE when the node rollup, the groups or the workload rows are off, when tails are asked for and
 * K20's SG_Q_NODES space is off, or while a flush is open: such a call leaves the stage as it was.  Memory is allocated here, never
 * at sg_create; a failed allocation (SG_ENOMEM) leaves the stage off.  Whatever frees one of its inputs frees this stage first:
 * sg_set_nodes(h, 0), any sg_set_groups call, sg_set_group_nodes(h, 0), and any sg_set_quantiles call when tails are on.
 * sg_group_assign does not touch it: each window is judged under the map it was contracted under.                               */
int sg_set_replicas(sg_handle h, const sg_replica_params* p);
/* The pod rows / workload rows of the last READ window, with sg_window_node_slo's shape: index NULL: every row, *n = their count;
 * else out[k] = the row of index[k] (each < the count, else SG_EINVAL), *n = n_index.  cap counts rows of SG_REPLICA_WORDS /
 * SG_REPLICA_GROUP_WORDS words; min(*n, cap) rows are written.                                                                   */
int sg_window_replicas(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
int sg_window_group_replicas(sg_handle h, const uint32_t* node_index, size_t n_index, uint32_t* out, size_t cap, size_t* n);
/* The device rows (uint32_t[node rows][SG_REPLICA_WORDS], uint32_t[workload rows][SG_REPLICA_GROUP_WORDS]) of the window
 * sg_window_run closed last; either pointer may be NULL.                                                                         */
int sg_window_replicas_buffer(sg_handle h, void** d_pod_rows, void** d_group_rows);
/* Selection over the pod rows of the last READ window: `by` is one of SG_RSEL_ERR / _LAT / _TAIL / _SHARE ORed with exactly one of
 * SG_RSEL_IN / SG_RSEL_OUT, else SG_EINVAL.  A row's key is max(err_excess_q20, 0), lat_ratio_q10, max(tail_excess, 0) or
 * share_q10 of that side when it is judged; key 0 and sides that are not judged are never candidates.  The k largest keys >=
 * min_value are selected (k = 0: every such row), ties by node position; rows and indices as sg_window_nodes_top gives them, the
 * rows byte-identical to sg_window_nodes'.  "The 20 replicas furthest above their peers' error rate" is
 * sg_window_replicas_top(h, SG_RSEL_ERR | SG_RSEL_IN, 20, 1, ...).                                                               */
#define SG_RSEL_ERR    0u
#define SG_RSEL_LAT    1u
#define SG_RSEL_TAIL   2u
#define SG_RSEL_SHARE  3u
#define SG_RSEL_IN     4u       /* the in side: the calls the pod receives */
#define SG_RSEL_OUT    8u       /* the out side: the calls it makes */
int sg_window_replicas_top(sg_handle h, uint32_t by, uint32_t k, uint32_t min_value, sg_node_out* out, uint32_t* index, size_t cap, size_t* n_selected, size_t* n_rows);

/* The window close in two halves, for hosts whose feeders keep running (the aggregator's worker goroutines do): sg_flush_begin
 * marks the window boundary — it waits for the staging copies that began before it (at most one batch copy per feeder; sg_ingest
 * calls that arrive meanwhile wait that long too, then belong to the NEXT window), enqueues K1 pass B .. K5 and returns.
 * sg_flush_end / sg_flush_end_view wait for the pipeline and fetch the rows without holding the engine lock, on a stream of
 * their own: the rows leave over PCIe while the next window's events arrive (full duplex), and no feeder stands still for the
 * ~1.7 ms a C3 window's kernels + copy-out take.  One begin may be open at a time (SG_ESTATE otherwise); any thread may call
 * the end.  sg_flush_window / sg_flush_window_view are exactly begin + end.                                                   */
int sg_flush_begin(sg_handle h, uint64_t window_end_ms);
int sg_flush_end(sg_handle h, sg_edge_out* out, size_t cap, size_t* n);
int sg_flush_end_view(sg_handle h, const sg_edge_out** rows, size_t* n);

/* Enqueue-only form of the same pipeline (K2..K5 + reset, no copy-out, no host sync) for
 * callers that keep results on the device (sg_window_rows_buffer) or time the pipeline.         */
int sg_window_run(sg_handle h, void* stream);
int sg_window_rows_buffer(sg_handle h, void** d_rows);   /* device sg_edge_out[max_edges] of the window
                                                             sg_window_run closed last (valid until its slot is reused) */

/* The same pipeline in stages, so that a sharded driver can run its exchanges in between.
 * Order: close -> [allreduce node stats] -> features -> for l in 0..L-1 { layer(l) ->
 * [halo exchange of layer l+1 rows] } -> score -> read -> reset.
 * All stage calls enqueue on `stream` (NULL = engine stream) and do not synchronise.            */
int sg_window_close(sg_handle h, void* stream);      /* K2: canonical ids, CSR; K3a: partial node stats */
/* Sharded close: OBIP numbering must agree on every shard, so the driver gathers every shard's
 * raw outbound IPs (sg_window_obip_list fills a caller-owned device list + device count), concatenates
 * them into d_union_ips (device, capacity >= next_pow2(world * max_outbound_ips), duplicates
 * allowed) and passes the total count in *d_union_n (device).                                   */
int sg_window_obip_list(sg_handle h, uint32_t* d_list, uint32_t cap, uint32_t* d_n, void* stream);
int sg_window_close_sharded(sg_handle h, const uint32_t* d_union_ips, const uint32_t* d_union_n, void* stream);
/* Sharded close with no host round trip: d_gathered is the all-gather of every shard's
 * [count, ip, ip, ...] u32 buffer (sg_window_obip_list with d_list = buf + 1, d_n = buf), `stride` u32
 * per shard.                                                                                     */
int sg_window_close_gathered(sg_handle h, const uint32_t* d_gathered, uint32_t stride, uint32_t world, void* stream);
int sg_window_features(sg_handle h, void* stream);   /* K3b: node + edge features from reduced stats    */
int sg_window_layer(sg_handle h, uint32_t l, void* stream);  /* K4: rows with out-edges owned here + all rows without out-edges */
int sg_window_score(sg_handle h, void* stream);      /* K5 */
int sg_window_score_reset(sg_handle h, void* stream);/* K5 with the window reset folded in (one launch less): for drivers
                                                        that read the rows through sg_window_rows_buffer(), not
                                                        sg_window_read(); the window is open again afterwards      */
int sg_window_read(sg_handle h, sg_edge_out* out, size_t cap, size_t* n); /* device-syncs, copies out; also valid after
                                                        sg_window_score_reset / sg_window_run_sharded until the next ingest */
int sg_window_reset(sg_handle h, void* stream);      /* clears the window state                  */

/* Device buffers a sharded driver reduces / exchanges (all device pointers, engine-owned):
 *  stats_sum: [n_nodes_cap][SG_NODE_STAT_SUM_WORDS] u64, SUM-reduce across shards
 *  stats_max: [n_nodes_cap][SG_NODE_STAT_MAX_WORDS] u64, MAX-reduce across shards
 *  counters : [8] u64 — {n_known, n_labels, n_obip, n_edges, n_events, dropped_src, dropped_cap, 0}
 *  feat(l)  : [n_nodes_cap][SG_F_HID] fp32 rows of layer l output (l = 1..L); l = 0 gives the
 *             [n_nodes_cap][SG_F_IN] input features.                                           */
int sg_window_buffers(sg_handle h, void** stats_sum, void** stats_max, void** counters,
                      size_t* n_nodes_cap);
int sg_window_feat_buffer(sg_handle h, uint32_t l, void** rows, size_t* row_floats);

/* Caller-owned device memory for the buffers a sharded driver reduces / exchanges in place
 * (stats_sum [ncap][SG_NODE_STAT_SUM_WORDS] u64, stats_max [ncap][2] u64, feat_rows[l] = layer l+1 rows [ncap][64] f32).
 * NULL entries keep the engine's own buffer.                                                    */
int sg_bind_buffers(sg_handle h, void* stats_sum, void* stats_max, void* const* feat_rows, uint32_t n_feat);

/* Halo support (K6).  Fill `ids` (device, u32[cap]) with the dense node indices this shard needs
 * from other shards — destinations of local edges that are not owned here and have out-edges —
 * grouped by owner shard (ascending id inside a group); counts[k] (device, u32[world]) = number
 * of ids owned by shard k.  pack/unpack move rows of layer l between the feature buffer and a
 * contiguous exchange buffer.  Call after the node statistics have been reduced.                */
int sg_halo_build(sg_handle h, uint32_t* d_ids, uint32_t cap, uint32_t* d_counts, void* stream);
/* Padded variants for a fixed-size all-to-all (no host synchronisation): lists are [world][capp + 1]
 * u32, element 0 = count.  Requests beyond capp are dropped and counted in sg_stats.halo_overflow.   */
int sg_halo_build_padded(sg_handle h, uint32_t* d_req, uint32_t capp, void* stream);
int sg_halo_pack_padded(sg_handle h, uint32_t l, const uint32_t* d_serve, uint32_t capp, float* d_rows, void* stream);
int sg_halo_unpack_padded(sg_handle h, uint32_t l, const uint32_t* d_req, uint32_t capp, const float* d_rows, void* stream);
int sg_halo_pack(sg_handle h, uint32_t l, const uint32_t* d_ids, uint32_t n, float* d_rows, void* stream);
int sg_halo_unpack(sg_handle h, uint32_t l, const uint32_t* d_ids, uint32_t n, const float* d_rows, void* stream);

/* ---- the sharded window in ONE call ------------------------------------------------------------------------------------ *
 * sg_window_run_sharded = sg_window_obip_list .. sg_window_score_reset above with every exchange in between — all-gather of
 * the raw outbound IPs, SUM / MAX all-reduce of the integer node statistics, all-to-all of the halo request lists, per layer
 * an all-to-all of exactly the requested rows — issued by the library itself on RCCL (grouped ncclSend / ncclRecv over the
 * xGMI full mesh) and enqueued on `stream`: one C call per window, nothing waits for the device, the exchange buffers belong
 * to the engine.  The communicator: rank 0 calls sg_comm_unique_id, the caller broadcasts the 128 bytes (any transport),
 * every rank calls sg_comm_create with its sg_config.rank / world.  RCCL is dlopen'ed (SG_ENODEV if it cannot be).      */
typedef struct sg_comm sg_comm;
int sg_comm_probe(void);                         /* SG_OK when librccl can be loaded with every symbol the library uses: lets all ranks agree
                                                    on a fallback BEFORE any of them enters ncclCommInitRank (which would wait for the others) */
int sg_comm_unique_id(void* id128, size_t bytes);
int sg_comm_create(const void* id128, size_t bytes, int rank, int world, int device, sg_comm** out);
int sg_comm_destroy(sg_comm* c);
int sg_window_run_sharded(sg_handle h, sg_comm* comm, void* stream);
/* Rows this shard asked each owner rank for in its last sharded window (counts[r], r < world).  Diagnostic; device-syncs. */
int sg_window_halo_counts(sg_handle h, uint32_t* counts, size_t world);

/* Ascending raw IPs of the last read window's OBIP nodes.                                       */
int sg_window_outbound_ips(sg_handle h, uint32_t* ips, size_t cap, size_t* n);
/* The latency histograms of the last read window (SG_CFG_EDGE_HISTOGRAM): bins[i * SG_HIST_BINS + b] = requests of row i in
 * bin b, rows in the order sg_flush_window / sg_window_read returned them.  *n = rows available.  SG_ESTATE without the flag. */
int sg_window_hist(sg_handle h, uint32_t* bins, size_t cap_rows, size_t* n);

int sg_stats_get(sg_handle h, sg_stats* out);

/* What sg_create chose for K1 (diagnostic: bench.py and the tuning scripts name the kernels they time with it). */
typedef struct sg_geometry {
    uint32_t k1_variant;        /* 0 partitioned aggregation, 1 global table + atomics                                      */
    uint32_t k1_narrow;         /* variant 0: 1 = 8-byte records (k1a_tile_partition / k1b_stream_merge), 0 = 16-byte records */
    uint32_t partitions;        /* np                                                                                        */
    uint32_t table_slots;       /* pass B: LDS table slots per partition                                                     */
    uint32_t pass_a_workgroups; /* pieces per partition                                                                      */
    uint32_t cache_slots;       /* pass A: LDS edge-cache slots (follows the join tables' size)                              */
    uint32_t join_l2_in_lds;    /* pass A: level 2 of the join staged in LDS (1) or read from global memory (0)              */
    uint32_t tile_records;      /* narrow: records sorted per tile                                                           */
    uint32_t endpoint_bits;     /* narrow: nb; remainder bits = 2 nb - log2(partitions)                                      */
    uint32_t piece_bytes;       /* record slab bytes per (partition, workgroup) piece                                        */
    uint32_t pass_b_split;      /* narrow: pass-B workgroups (sub-tables) per partition                                      */
    uint32_t pass_a_teams;      /* narrow: k1a_team_partition with 2 teams of eight waves per workgroup or 1 team of sixteen; 0 = k1a_tile_partition */
    uint32_t warm_windows;      /* 1 = the engine carries the edge set and its CSR order from window to window (SG_CFG_NO_WARM)   */
} sg_geometry;
int sg_geometry_get(sg_handle h, sg_geometry* out);
/* The close's launch plan, beside sg_geometry (whose layout is fixed): *out = 1 when a window close that tries the warm path launches no
 * kc_prepare — that kernel's work rides in the warm attempt's launch (unsharded engines that keep warm-window state). */
int sg_prepare_fold_get(sg_handle h, uint32_t* out);
/* Pass A's tile pairs, beside sg_geometry likewise: *out = 1 when a team of k1a_team_partition copies two tiles of tile_records records out
 * together (runs of twice the length per partition).  Follows the join tables like the rest of pass A's geometry. */
int sg_pass_a_pair_get(sg_handle h, uint32_t* out);
/* The score kernel's form, beside sg_geometry likewise: *out = 0 when k5_edge_score gives sixteen lanes to an edge, 1 when one lane
 * owns an edge and the P and Q rows pass through LDS (k5_edge_score_lanes).  Both write the same rows, bit for bit. */
int sg_k5_form_get(sg_handle h, uint32_t* out);
/* Where the edge features are computed, beside sg_geometry likewise: *out = 0 when k3_node_features stores them for the score kernel,
 * 1 when k5_edge_score_lanes computes them for its own edge (form 1 only; the engine then holds no feature arrays).  Same rows, bit
 * for bit. */
int sg_k5_efeat_get(sg_handle h, uint32_t* out);
/* K3's forms, beside sg_geometry likewise: *in_form = 1 when k3_in_part issues all loads of a trip together (0: under their tests, one
 * by one), *feat_lanes = 1 when the node features run eight lanes per node (k3_node_features_lanes; node-only launches, i.e. beside
 * sg_k5_efeat_get = 1).  Same statistics and features, bit for bit. */
int sg_k3_forms_get(sg_handle h, uint32_t* in_form, uint32_t* feat_lanes);

/* Per-kernel timing, measured on the launch stream.  Groups: 1 = K1 pass A (k1a_partition / k1_resolve_aggregate, one record
 * per batch), 7 = K1 pass B (k1b_merge) — both by the dispatch's own begin/end stamps; 2 = K2 csr_build (two records per window:
 * window bookkeeping, then row pointers + scatter + row sort), 8 = K3 in-statistics, 3 = K3 node + edge features, 4 = K4 (one
 * record per SAGE layer), 5 = K5, 6 = K6 halo kernels, 9 = the collectives of sg_window_run_sharded (one record per RCCL call) — by hipEvent
 * pairs around the launches.  sg_timing_get returns the
 * average duration in microseconds per record since sg_timing_reset(), and the number of records.  An engine that keeps warm-window
 * state launches pass B twice per window (the warm attempt and the cold merge; one of them returns at once): group 7 then has two
 * records per window and a window's pass B is their sum.                                                                    */
int sg_timing_enable(sg_handle h, int on);   /* 0 = off, 1 = every group, else bitmask: bit k = group Kk */
int sg_timing_reset(sg_handle h);
int sg_timing_stride(sg_handle h, uint32_t n);   /* groups 1 and 7 (dispatch stamps, a few us per launch): on every n-th window only; 1 = every window */
int sg_timing_get(sg_handle h, int kernel, double* avg_us, uint64_t* launches);
/* Warm windows on / off at run time (on = 0: no window tries the warm path from now on, each is rebuilt and re-captured; on = 1: back
 * to the default).  The rows never depend on it; bench.py uses it to time the cold path beside the steady state.                     */
int sg_set_warm(sg_handle h, int on);
/* Every record of a group since sg_timing_reset, in launch order: min(*n, cap) durations in microseconds go to us[], *n = how many
 * there are.  Group 10 (only when its bit is set explicitly or with on = 1) = one record per window of sg_window_run /
 * sg_window_run_sharded, from in front of the window's first pass-A launch to behind its score kernel.                      */
int sg_timing_samples(sg_handle h, int kernel, double* us, size_t cap, size_t* n);
/* Memory latency of this box: one lane follows `steps` dependent loads (one 128-byte line each, an odd-multiplier walk over all
 * lines) through `bytes` of device memory it allocates for the call; *ns_per_load by the 100 MHz reference clock.  warm & 1
 * walks every line once before the clock starts (a 2 MiB buffer then measures the L2, a buffer far beyond the 256 MiB Infinity
 * Cache without it measures HBM); warm & 2: 65 536 lanes follow a chain each at the same time and one of them is timed — the
 * latency of a random line under load.  Diagnostic for bench.py ("which kind of box did this line come from"); device-syncs.  */
int sg_latency_probe(sg_handle h, uint64_t bytes, uint32_t steps, int warm, double* ns_per_load);
/* The shader clock the chip sustains, in MHz (shader cycles per 100 MHz reference tick x 100): *spin_mhz from an all-CU integer
 * spin of about spin_us microseconds launched by this call, *k1a_mhz averaged over the K1 pass-A launches since the previous
 * call (0 if none; narrow-record kernels only).  Diagnostic for bench.py: the boxes of a pool differ in the clock they hold
 * under load.  Device-syncs.                                                                                               */
int sg_clock_probe(sg_handle h, uint32_t spin_us, double* spin_mhz, double* k1a_mhz);
/* Tuning aid: with SG_ABLATE & 0x100 in the environment at sg_create, the K1 kernels record 100 MHz
 * wall-clock stamps at their phase boundaries, [kernel 0..3][4096 workgroups][8 stamps] u64; this
 * copies the first n words out.  All zero otherwise.                                                */
int sg_debug_stamps(sg_handle h, uint64_t* out, size_t n);

/* Owner shard of a node / routing shard of an event: murmur3 fmix32(ip) % world.
 * The feeder routes an event by the IP of its from-endpoint: daddr if SG_EV_REVERSE (and not SG_EV_ALIVE) else saddr. */
uint32_t sg_hash32(uint32_t x);
/* Shard each event must be fed to when world > 1: owner of its from-endpoint after the join and
 * the optional direction reversal — the same rule K1 enforces (misrouted events are dropped and
 * counted).  Host-only: uses the host mirror of the join tables, launches nothing.              */
int sg_route(sg_handle h, const sg_event* events, size_t n, uint32_t world, uint32_t* shard_out);

#ifdef __cplusplus
}
#endif
#endif /* SERVICEGRAPH_H */
