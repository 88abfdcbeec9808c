// graph_ds.hpp — GraphDS: a datastore.DataStore decorator that feeds the MI355X ServiceGraph engine.
//
// It is what INTEGRATION.md's Go `GraphDS` is, written in C++ because no Go toolchain exists in the
// build environment: it wraps an inner DataStore (the reference's BackendDS), forwards the eight k8s
// resource calls unchanged, mirrors pod / service IP changes into the engine's join tables
// (sg_upsert_* / sg_delete_*, the analogue of aggregator/persist.go:55-71,114-130), turns the per-request
// calls into packed events (sg_ingest) and, once per window, reads back one scored row per edge
// (sg_flush_window) and hands them to an EdgeSink.
//
// Two taps exist, as in SURVEY.md §8b:
//   * PersistRequest / PersistKafkaEvent — the datastore boundary itself (the reference aggregator has
//     already run setFromToV2; the engine repeats the join on the GPU from FromIP / ToIP);
//   * IngestL7 — one step earlier, straight from l7_req.L7Event, so that the reference's CPU join is
//     not needed at all (the L7Packer does the payload-dependent part on the host).
#pragma once
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/servicegraph.h"
#include "datastore.hpp"
#include "l7_event.hpp"
#include "packer.hpp"

namespace alaz {

// the C ABI as a table of function pointers: the real library (dlsym) in production, a recording
// stand-in in the host-logic tests.
struct SgApi {
    int (*create)(const sg_config*, sg_handle*) = nullptr;
    int (*destroy)(sg_handle) = nullptr;
    int (*upsert_pod)(sg_handle, uint32_t, uint32_t) = nullptr;
    int (*delete_pod)(sg_handle, uint32_t) = nullptr;
    int (*upsert_service)(sg_handle, uint32_t, uint32_t) = nullptr;
    int (*delete_service)(sg_handle, uint32_t) = nullptr;
    int (*set_label_count)(sg_handle, uint32_t) = nullptr;
    int (*ingest)(sg_handle, const sg_event*, size_t) = nullptr;
    int (*flush_window)(sg_handle, uint64_t, sg_edge_out*, size_t, size_t*) = nullptr;
    int (*flush_window_view)(sg_handle, uint64_t, const sg_edge_out**, size_t*) = nullptr;   // optional (absent in a recording stand-in): rows stay in the engine's pinned buffer
    int (*window_outbound_ips)(sg_handle, uint32_t*, size_t, size_t*) = nullptr;
    int (*flush_window_top)(sg_handle, uint64_t, uint32_t, float, sg_edge_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;   // optional: SetSelection needs it
    const char* (*last_error)(sg_handle) = nullptr;
    // optional (K14; absent in an older library): SetWorkloadGroups needs the first two, WorkloadEdges the third
    int (*set_groups)(sg_handle, const sg_group_params*) = nullptr;
    int (*group_assign)(sg_handle, const uint32_t*, const uint32_t*, size_t) = nullptr;
    int (*window_groups)(sg_handle, sg_group_edge*, size_t, size_t*) = nullptr;
    // optional (K15; absent in an older library): each of SetWorkloadTrend, SetWorkloadVanished, WorkloadTrends, WorkloadVanished and
    // WorkloadTop needs the entry it forwards to
    int (*set_group_trend)(sg_handle, const sg_trend_params*) = nullptr;
    int (*window_group_trend)(sg_handle, const uint32_t*, size_t, sg_edge_trend*, size_t, size_t*) = nullptr;
    int (*set_group_vanished)(sg_handle, const sg_vanished_params*) = nullptr;
    int (*window_group_vanished)(sg_handle, sg_edge_vanished*, size_t, size_t*) = nullptr;
    int (*window_groups_top)(sg_handle, uint32_t, uint32_t, float, sg_group_edge*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K16; absent in an older library): each of SetWorkloadNodes, WorkloadNodes, SetWorkloadNodeTrend, WorkloadNodeTrends
    // and WorkloadNodesTop needs the entry it forwards to
    int (*set_group_nodes)(sg_handle, int) = nullptr;
    int (*window_group_nodes)(sg_handle, sg_node_out*, size_t, size_t*) = nullptr;
    int (*set_group_node_trend)(sg_handle, const sg_trend_params*) = nullptr;
    int (*window_group_node_trend)(sg_handle, const uint32_t*, size_t, sg_node_trend*, size_t, size_t*) = nullptr;
    int (*window_group_nodes_top)(sg_handle, uint32_t, uint32_t, float, sg_node_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K17; absent in an older library): SetWorkloadRank and WorkloadCulprits each need the entry they forward to
    int (*set_group_rank)(sg_handle, const sg_rank_params*) = nullptr;
    int (*window_group_rank_top)(sg_handle, uint32_t, float, sg_node_out*, sg_node_rank*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K18; absent in an older library): SetWorkloadIncidents and WorkloadIncidents each need the entry they forward to
    int (*set_group_incidents)(sg_handle, const sg_incident_params*) = nullptr;
    int (*window_group_incidents)(sg_handle, sg_incident_out*, size_t, size_t*) = nullptr;
    int (*window_group_node_incident)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*) = nullptr;
    // optional (K19; absent in an older library): SetWorkloadTracks, WorkloadIncidentTracks and WorkloadTracksEnded each need the
    // entry they forward to
    int (*set_group_tracks)(sg_handle, const sg_track_params*) = nullptr;
    int (*window_group_incident_tracks)(sg_handle, sg_incident_track*, size_t, size_t*) = nullptr;
    int (*window_group_tracks_ended)(sg_handle, sg_track_entry*, size_t, size_t*) = nullptr;
    // optional (K22; absent in an older library): SetWorkloadImpact and WorkloadImpact each need the entry they forward to
    int (*set_group_impact)(sg_handle, uint32_t, uint32_t) = nullptr;
    int (*window_group_impact)(sg_handle, uint64_t*, size_t, size_t*) = nullptr;
    // optional (K20; absent in an older library): SetQuantiles and the three latency reads each need the entry they forward to
    int (*set_quantiles)(sg_handle, uint32_t, const uint32_t*, size_t) = nullptr;
    int (*window_node_quantiles)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*) = nullptr;
    int (*window_group_quantiles)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*) = nullptr;
    int (*window_group_node_quantiles)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*) = nullptr;
    // optional (K21; absent in an older library): SetTailTrend, the three tail reads and WorkloadTailTop each need the entry they forward to
    int (*set_quantile_trend)(sg_handle, uint32_t, uint32_t, const sg_trend_params*) = nullptr;
    int (*window_node_quantile_trend)(sg_handle, const uint32_t*, size_t, sg_node_trend*, size_t, size_t*) = nullptr;
    int (*window_group_quantile_trend)(sg_handle, const uint32_t*, size_t, sg_edge_trend*, size_t, size_t*) = nullptr;
    int (*window_group_node_quantile_trend)(sg_handle, const uint32_t*, size_t, sg_node_trend*, size_t, size_t*) = nullptr;
    int (*window_group_nodes_top_tail)(sg_handle, uint32_t, uint32_t, float, sg_node_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K23; absent in an older library): SetTrafficTrend and WorkloadTrafficTop each need the entry they forward to
    int (*set_traffic_trend)(sg_handle, uint32_t, const sg_traffic_params*) = nullptr;
    int (*window_group_nodes_top_traffic)(sg_handle, uint32_t, uint32_t, float, sg_node_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K24; absent in an older library): SetSLO, SetWorkloadSLO, WorkloadSLO and WorkloadSLOTop each need the entry they forward to
    int (*set_slo)(sg_handle, uint32_t, const sg_slo_params*) = nullptr;
    int (*slo_assign)(sg_handle, uint32_t, const uint32_t*, const uint32_t*, size_t) = nullptr;
    int (*window_group_node_slo)(sg_handle, const uint32_t*, size_t, uint64_t*, size_t, size_t*) = nullptr;
    int (*window_group_nodes_top_slo)(sg_handle, uint32_t, uint32_t, uint32_t, sg_node_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    // optional (K25; absent in an older library): SetReplicaOutliers and WorkloadReplicaOutliers each need the entries they forward to
    int (*set_replicas)(sg_handle, const sg_replica_params*) = nullptr;
    int (*window_replicas)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*) = nullptr;
    int (*window_replicas_top)(sg_handle, uint32_t, uint32_t, uint32_t, sg_node_out*, uint32_t*, size_t, size_t*, size_t*) = nullptr;
    static bool FromLibrary(void* dl_handle, SgApi* out);      // dlsym of every entry; false if one is missing
};

struct EdgeRow {                       // one edge of a closed window, in the reference's vocabulary
    std::string FromType, FromUID, ToType, ToUID;
    uint32_t Count = 0, ErrCount = 0;
    uint64_t SumNs = 0, MaxNs = 0, SumSqUs = 0;
    float Score = 0, LatZ = 0, ErrRatio = 0;
    uint32_t Alive = 0;                // open connections reported on the edge in the window
    uint32_t P50Us = 0, P99Us = 0;     // latency percentiles off the edge's log2 histogram (0 unless SG_CFG_EDGE_HISTOGRAM)
};

struct WorkloadEdge {                  // one edge of a closed window's service map contracted to workloads (sg_group_edge)
    std::string FromType, FromUID, ToType, ToUID;      // type "workload": the UID of the pod's top known owner; else as EdgeRow
    uint64_t Count = 0, ErrCount = 0, SumNs = 0, SumSqUs = 0, MaxNs = 0, ScoreQ32 = 0;
    uint32_t Edges = 0, FromNodes = 0, Alive = 0, WorstRow = 0;
    float ScoreMax = 0;
};

struct VanishedWorkload {              // one vanished workload dependency of a closed window (sg_edge_vanished over workload keys)
    uint64_t FromKey = 0, ToKey = 0;                   // the workload keys (include/servicegraph.h, "workload baselines")
    std::string FromUID, ToUID;                        // key type 0 (a workload): the owner's UID; any other key type: empty, the key stands
    double LatMean = 0, LatDev = 0, ErrMean = 0, ErrDev = 0;
    uint32_t N = 0, Last = 0, Row = 0;                 // Row: the window's group edge with the key and no request, else 0xFFFFFFFF
};

struct ReplicaOutlier {                // one selected replica of a closed window (K25): who it is, whose replica, and one side of its pod row
    std::string PodUID, Workload;      // the pod's UID; the owner UID of its workload
    uint32_t NodeIndex = 0, WorkloadIndex = 0;   // into ServiceNodes' / WorkloadNodes' rows of the window
    uint32_t Flags = 0;                // word 1 of the pod row: SG_REPL_* of both sides
    int32_t ErrExcessQ20 = 0;          // the side `by` names: error rate above the peers', 2^20 = 100 points
    uint32_t LatRatioQ10 = 0, ShareQ10 = 0, TailPod = 0, TailPeers = 0, Replicas = 0;   // mean over the peers' mean, share of the fair share (1024 = 1); K20 bins; R
};
struct WorkloadNode {                  // one workload row of a closed window (K16): who it is, and the engine's row as it is
    std::string Type, UID;                             // "workload" (UID = the owner's UID), or pod / service / outbound as the rows' are
    sg_node_out Row{};
};

struct WorkloadCulprit {               // one selected workload of a closed window's ranking (K17): the workload row named, and its rank row
    WorkloadNode Node;
    sg_node_rank Rank{};
};

class EdgeSink {
public:
    virtual ~EdgeSink() = default;
    virtual int PersistEdges(int64_t window_end_ms, const std::vector<EdgeRow>& rows) = 0;
};

bool ParseIPv4(const std::string& s, uint32_t* out);     // "a.b.c.d" -> a<<24|b<<16|c<<8|d
std::string FormatIPv4(uint32_t ip);                      // IntToIPv4().String(), aggregator/data.go:1751-1758

class GraphDS : public datastore::DataStore {
public:
    // max_known_nodes = sg_config.max_known_nodes (the id space the engine was created with).  divert_requests: false
    // (default) = additive — PersistRequest / PersistKafkaEvent also reach the inner data store, so a backend without an
    // "/edges/" route keeps receiving its per-request rows; true = the engine's per-edge rows replace them.
    GraphDS(datastore::DataStore* inner, const SgApi& api, sg_handle h, EdgeSink* sink, size_t max_edges, size_t batch = 4096,
            uint32_t max_known_nodes = 0x3FFFFFFFu, bool divert_requests = false);
    ~GraphDS() override;

    int PersistPod(const datastore::Pod& pod, const std::string& eventType) override;
    int PersistService(const datastore::Service& service, const std::string& eventType) override;
    // forwarded; with the workload groups on, a ReplicaSet that names a Deployment moves its pods into the Deployment's group
    int PersistReplicaSet(const datastore::ReplicaSet& rs, const std::string& et) override;
    int PersistDeployment(const datastore::Deployment& d, const std::string& et) override { return inner_->PersistDeployment(d, et); }
    // forwarded unchanged; the pods behind (namespace, name) are remembered for SetServiceBinding
    int PersistEndpoints(const datastore::Endpoints& e, const std::string& et) override;
    int PersistContainer(const datastore::Container& c, const std::string& et) override { return inner_->PersistContainer(c, et); }
    int PersistDaemonSet(const datastore::DaemonSet& ds, const std::string& et) override { return inner_->PersistDaemonSet(ds, et); }
    int PersistStatefulSet(const datastore::StatefulSet& ss, const std::string& et) override { return inner_->PersistStatefulSet(ss, et); }
    int PersistRequest(const datastore::Request* request) override;
    int PersistKafkaEvent(const datastore::KafkaEvent* request) override;
    // an open TCP connection (sendOpenConnection, data.go:1628-1679): forwarded, and fed to the engine as an
    // SG_EV_ALIVE record — the join (source must be a pod, service before pod, else the IP) runs on the GPU
    int PersistAliveConnection(const datastore::AliveConnection* conn) override;

    // earlier tap: the raw L7 event (what processL7 receives, aggregator/data.go:1364-1383)
    int IngestL7(const l7_req::L7Event& e, uint32_t kafka_msgs = 1);
    // n perf records of l7_req::kWireSize bytes each, through L7Packer::PackWire (f-1: no 1 KiB copy per event)
    int IngestWire(const uint8_t* recs, size_t n, const uint32_t* kafka_msgs = nullptr);

    // process / connection lifecycle as far as the payload parsers need it (aggregator/data.go:354-401, :484-503,
    // :553-567): only events of live pids are assembled; a closed connection or an exited process drops its HPACK state
    // and its remembered Postgres statements
    void ProcExec(uint32_t pid) { std::lock_guard<std::mutex> g(pk_mu_); packer_.Http2().ProcExec(pid); }
    void ProcExit(uint32_t pid) { std::lock_guard<std::mutex> g(pk_mu_); packer_.ProcExit(pid); }
    void ConnClosed(uint32_t pid, uint64_t fd) { std::lock_guard<std::mutex> g(pk_mu_); packer_.ConnClosed(pid, fd); }
    void SetKafkaDecode(bool on) { std::lock_guard<std::mutex> g(pk_mu_); packer_.SetKafkaDecode(on); }
    void SweepHttp2() { std::lock_guard<std::mutex> g(pk_mu_); packer_.Http2().Sweep(); }

    // close the window: pending batches -> engine, K2..K5, rows -> sink.  Returns the number of edges or < 0.
    long FlushWindow(int64_t window_end_ms);
    // From the next FlushWindow on, only the window's selected rows go to the sink, in selection order (sg_flush_window_top: k = 0
    // every row scoring >= min_score in canonical order, else the k highest-scoring of them); FlushWindow still returns the
    // window's edge count.  SG_EINVAL for k > SG_SELECT_MAX_K or an engine without sg_flush_window_top.  ClearSelection: all rows.
    int SetSelection(uint32_t k, float min_score);
    void ClearSelection() { std::lock_guard<std::mutex> g(flush_mu_); select_ = false; }

    // The workload view (sg_set_groups, K14): every pod is assigned to the group of its top known owner — Pod.OwnerID; if that is a
    // ReplicaSet with a known OwnerID, that Deployment; DaemonSet / StatefulSet owners as they are; a pod without an owner stays
    // ungrouped.  Owner UIDs are interned to group ids in arrival order (max_groups of them, 0 = max_known_nodes; an owner beyond
    // them leaves its pods ungrouped and counts as an engine error).  sg_group_assign follows every pod upsert; a deleted pod
    // leaves its group when its node id is released, after the window that may still name it has been flushed; a ReplicaSet that
    // arrives after its pods re-assigns them.  SG_EINVAL without sg_set_groups / sg_group_assign in the engine's table.
    int SetWorkloadGroups(uint32_t max_groups);
    // Service binding (off by default; needs SetWorkloadGroups, else SG_ESTATE; SG_EINVAL without sg_group_assign): a Service's node
    // id joins the workload behind it, so that pod -> ClusterIP traffic contracts to workload -> workload and call chains run
    // through Services.  (namespace, name) -> Service comes from PersistService, (namespace, name) -> pod UIDs from PersistEndpoints
    // (the addresses of Type "Pod" with a non-empty ID); DELETE forgets the entry.  A Service is in group g iff its Endpoints name
    // at least one pod that has an IP here, and every such pod is in the same group g (two ReplicaSets of one Deployment are one
    // g); otherwise — no Endpoints, no known pod, an ungrouped pod among them, two workloads behind it — it is in none.  The rule is
    // re-evaluated whenever an input changes (an Endpoints or Service event, a pod added, removed or re-owned, a ReplicaSet's owner
    // learned, SetWorkloadGroups, this switch) and sent as one sg_group_assign only when the value changes; off un-assigns every
    // bound Service.  A window already in flight keeps the map it was closed under.
    int SetServiceBinding(bool on);
    // the group edges of the last flushed window, group ids resolved back to owner UIDs; < 0 on an engine error
    long WorkloadEdges(std::vector<WorkloadEdge>* out);
    // The workload baselines (K15), behind SetWorkloadGroups: each group edge against its own past, keyed by workload, so a rollout
    // (new pods, new ids) keeps the history.  The two switches forward sg_set_group_trend / sg_set_group_vanished (the engine's
    // return code; SG_EINVAL without the entry).  WorkloadTrends: row k for edge k of WorkloadEdges.  WorkloadTop: the selection
    // sg_window_groups_top over the last flushed window (`by` = SG_SEL_*), the edges resolved as WorkloadEdges does, their indices
    // in `index` (may be NULL) — what WorkloadTrends' rows are indexed by.  WorkloadVanished: the window's vanished workload
    // dependencies, key type 0 resolved back to the owner's UID through the group table SetWorkloadGroups built.  Each returns
    // the count (WorkloadTop: the selected edges; WorkloadVanished: the rows the list holds), < 0 on an engine error.
    int SetWorkloadTrend(const sg_trend_params& p);
    int SetWorkloadVanished(const sg_vanished_params& p);
    long WorkloadTrends(std::vector<sg_edge_trend>* out);
    long WorkloadTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadEdge>* out, std::vector<uint32_t>* index);
    long WorkloadVanished(std::vector<VanishedWorkload>* out);
    // The workload rows (K16), behind SetWorkloadGroups: the last flushed window's group edges rolled up per workload, in the order
    // of the group key (the workloads first).  SetWorkloadNodes / SetWorkloadNodeTrend forward sg_set_group_nodes /
    // sg_set_group_node_trend (the engine's return code; SG_EINVAL without the entry).  WorkloadNodes: one row per workload, group
    // ids resolved back to owner UIDs as WorkloadEdges does.  WorkloadNodeTrends: row k for row k of WorkloadNodes.
    // WorkloadNodesTop: the selection sg_window_group_nodes_top (`by` = SG_NSEL_*), the rows' indices in `index` (may be NULL).
    // Each returns the count, < 0 on an engine error.
    int SetWorkloadNodes(bool on);
    int SetWorkloadNodeTrend(const sg_trend_params& p);
    long WorkloadNodes(std::vector<WorkloadNode>* out);
    long WorkloadNodeTrends(std::vector<sg_node_trend>* out);
    long WorkloadNodesTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index);
    // The workload ranking (K17), behind SetWorkloadNodes: the last flushed window's likely root-cause workloads.  SetWorkloadRank
    // forwards sg_set_group_rank (p NULL: off; the engine's return code; SG_EINVAL without the entry).  WorkloadCulprits: the
    // selection sg_window_group_rank_top — the rows named as WorkloadNodes names them, each with its rank row, the rows' indices in
    // `index` (may be NULL).  It returns the count, < 0 on an engine error.
    int SetWorkloadRank(const sg_rank_params* p);
    long WorkloadCulprits(uint32_t k, float min_share, std::vector<WorkloadCulprit>* out, std::vector<uint32_t>* index);
    // The workload incidents (K18), behind SetWorkloadNodes: the last flushed window's red group edges grouped into connected
    // components of workload rows.  SetWorkloadIncidents forwards sg_set_group_incidents (p NULL: off; the engine's return code;
    // SG_EINVAL without the entry).  WorkloadIncidents: the incident rows (first_node, top_node and culprit_node index
    // WorkloadNodes, worst_row indexes WorkloadEdges) and, in `node_incident` (may be NULL), the incident of every row of
    // WorkloadNodes (SG_NO_INCIDENT: none).  It returns the incident count, < 0 on an engine error.
    int SetWorkloadIncidents(const sg_incident_params* p);
    long WorkloadIncidents(std::vector<sg_incident_out>* out, std::vector<uint32_t>* node_incident);
    // The workload tracks (K19; needs SetWorkloadIncidents): the workload incidents followed across windows, so that an incident keeps
    // its id through a rollout.  SetWorkloadTracks forwards sg_set_group_tracks (p NULL: off; the engine's return code; SG_EINVAL
    // without the entry).  WorkloadIncidentTracks: row i is the track of WorkloadIncidents' row i of the last flushed window;
    // WorkloadTracksEnded: the tracks that went quiet in it, as they stood.  Both: the count, or a negative SG_* code.
    int SetWorkloadTracks(const sg_track_params* p);
    long WorkloadIncidentTracks(std::vector<sg_incident_track>* out);
    long WorkloadTracksEnded(std::vector<sg_track_entry>* out);
    // The workload impact (K22; needs SetWorkloadIncidents): who depends on each workload incident.  SetWorkloadImpact forwards
    // sg_set_group_impact (0, 0: off; the engine's return code; SG_EINVAL without the entry).  WorkloadImpact: the last flushed
    // window's incident rows as WorkloadIncidents gives them and, in `impact`, SG_IMPACT_WORDS words per covered incident — row i
    // belongs to incident i; the row in FAR's low half indexes WorkloadNodes.  It returns the covered count, or a negative SG_* code.
    int SetWorkloadImpact(uint32_t max_incidents, uint32_t max_hops);
    long WorkloadImpact(std::vector<sg_incident_out>* incidents, std::vector<uint64_t>* impact);
    // The latency percentiles (K20; the engine was created with SG_CFG_EDGE_HISTOGRAM): SetQuantiles forwards sg_set_quantiles
    // (spaces: SG_Q_* bits, 0 = off; n_q 0: {500, 990}; the engine's return code; SG_EINVAL without the entry).  NodeLatency,
    // WorkloadEdgeLatency and WorkloadLatency read the last flushed window's quantiles in microseconds — per node row [2][n_q]
    // (out side, in side), per group edge [n_q], per workload row [2][n_q] — of every entity (index NULL) or of those at index,
    // into out_us; they return the entity count, or a negative SG_* code.
    int SetQuantiles(uint32_t spaces, const uint32_t* permille, size_t n_q);
    long NodeLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us);
    long WorkloadEdgeLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us);
    long WorkloadLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us);
    // The tail baselines (K21; behind SetQuantiles over the same spaces): each entity's tracked quantile against its own past.
    // SetTailTrend forwards sg_set_quantile_trend (spaces: SG_Q_* bits, 0 or p NULL = off; permille: one of those SetQuantiles gave;
    // the engine's return code; SG_EINVAL without the entry).  NodeTailTrends, WorkloadEdgeTailTrends and WorkloadTailTrends read
    // the last flushed window's tail rows: row k for node row k, for edge k of WorkloadEdges, for row k of WorkloadNodes.
    // WorkloadTailTop: the selection sg_window_group_nodes_top_tail (`by` = SG_NSEL_*, ranked by the tail rows), its rows named as
    // WorkloadNodesTop names them, their indices in `index` (may be NULL).  Each returns the count, or a negative SG_* code.
    int SetTailTrend(uint32_t spaces, uint32_t permille, const sg_trend_params* p);
    long NodeTailTrends(std::vector<sg_node_trend>* out);
    long WorkloadEdgeTailTrends(std::vector<sg_edge_trend>* out);
    long WorkloadTailTrends(std::vector<sg_node_trend>* out);
    long WorkloadTailTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index);
    // The traffic baselines (K23): each entity's request rate and load against its own past.  SetTrafficTrend forwards
    // sg_set_traffic_trend (spaces: SG_T_* bits, 0 or p NULL = off; the engine's return code; SG_EINVAL without the entry).
    // WorkloadTrafficTop: the selection sg_window_group_nodes_top_traffic (`by` = SG_TSEL_SURGE .. SG_TSEL_LOAD_DOWN ORed with
    // SG_TSEL_IN or SG_TSEL_OUT: SG_TSEL_DROP | SG_TSEL_IN = the workloads whose inbound traffic fell furthest), its rows named as
    // WorkloadNodesTop names them, their indices in `index` (may be NULL).  Returns the count, or a negative SG_* code.
    int SetTrafficTrend(uint32_t spaces, const sg_traffic_params* p);
    long WorkloadTrafficTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index);
    // The SLO burn rates (K24; needs SetLatencyQuantiles for the space): each service's and workload's error budget over a short
    // and a long span of windows.  SetSLO forwards sg_set_slo (spaces: SG_Q_NODES | SG_Q_GROUP_NODES, 0 or p NULL = off; the engine's
    // return code; SG_EINVAL without the entry).  SetWorkloadSLO: the objective word (SG_SLO_OBJECTIVE; 0 = the defaults) of the
    // workload with this owner UID, SG_EINVAL for an owner no pod has named yet.  WorkloadSLO: the last flushed window's SLO rows,
    // SG_SLO_WORDS words a row, row k for row k of WorkloadNodes.  WorkloadSLOTop: the selection sg_window_group_nodes_top_slo
    // (`by` = SG_SLOSEL_ERR or SG_SLOSEL_SLOW ORed with SG_SLOSEL_IN or SG_SLOSEL_OUT; min_value_q10 in 1/1024 of "on budget"), its
    // rows named as WorkloadNodesTop names them, their indices in `index` (may be NULL).  The count, or a negative SG_* code.
    int SetSLO(uint32_t spaces, const sg_slo_params* p);
    int SetWorkloadSLO(const std::string& workload, uint32_t objective);
    long WorkloadSLO(std::vector<uint64_t>* out);
    long WorkloadSLOTop(uint32_t by, uint32_t k, uint32_t min_value_q10, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index);
    // The replica outliers (K25; needs the node rollup, SetWorkloadGroups and the workload rows, and SetLatencyQuantiles over the
    // services for tails): each pod against the other pods of its workload.  SetReplicaOutliers forwards sg_set_replicas (p NULL = off;
    // the engine's return code; SG_EINVAL without the entry).  WorkloadReplicaOutliers: the selection sg_window_replicas_top over the
    // last flushed window (`by` = SG_RSEL_ERR / _LAT / _TAIL / _SHARE ORed with SG_RSEL_IN or SG_RSEL_OUT), each selected pod named by
    // its UID and its workload's owner UID, with that side's words of its pod row.  The count, or a negative SG_* code.
    int SetReplicaOutliers(const sg_replica_params* p);
    long WorkloadReplicaOutliers(uint32_t by, uint32_t k, uint32_t min_value, std::vector<ReplicaOutlier>* out);

    uint64_t EventsOffered() const { return offered_.load(); }
    uint64_t BatchesDropped() const { return batches_dropped_.load(); }
    uint64_t EngineErrors() const { return engine_errors_.load(); }   // sg_upsert_* failures (SG_ENOSPC: id space / join table full)
    size_t LiveIds() const { return live_ids_; }
    const std::vector<std::string>& Labels() const { return packer_.Labels(); }
    const L7Packer& Packer() const { return packer_; }

private:
    static constexpr uint32_t kNoId = 0xFFFFFFFFu;
    static constexpr int kShards = 8;
    struct Shard { std::mutex mu; std::vector<sg_event> batch; };

    // node ids (under id_mu_): one per UID that currently owns at least one IP in the join tables.  An id whose last IP
    // is gone is retired, and handed out again once the window that may still name it has been flushed.
    uint32_t Intern(const std::string& uid, uint8_t kind);            // kNoId when the id space is exhausted
    void BindIP(std::unordered_map<uint32_t, uint32_t>& m, uint32_t ip, uint32_t id);   // m[ip] = id, reference counts follow
    void UnbindIP(std::unordered_map<uint32_t, uint32_t>& m, uint32_t ip);
    int Append(const sg_event* ev, size_t n);
    // (id_mu_ held) the group of a pod owned by `owner` (kNoId: none); node id -> group in the engine, if it changed
    uint32_t GroupOfOwner(const std::string& owner);
    void AssignGroup(uint32_t id, uint32_t group);
    // (id_mu_ held) the binding rule for the Service at key "namespace/name"; for every Service whose Endpoints name the pod; for all
    void BindService(const std::string& key);
    void BindServicesOfPod(const std::string& pod_uid);
    void BindAllServices();
    // (id_mu_ held) a group edge in the reference's vocabulary: group ids back to owner UIDs, node refs as the rows' are
    void NameWorkloadEdge(const sg_group_edge& r, WorkloadEdge* o) const;
    void NameRef(uint32_t ref, std::string* type, std::string* uid) const;   // (id_mu_ held) one group ref
    void NameWorkloadNodes(const std::vector<sg_node_out>& rows, std::vector<WorkloadNode>* out);   // (takes id_mu_)
    int FlushShard(Shard& s);                          // s.mu held
    // a selection over the workload rows through `top` (sg_window_group_nodes_top or its _tail twin): WorkloadNodesTop's body
    // (V: the threshold's type — float, or K24's uint32_t)
    template <class V>
    long WorkloadNodesTopBy(int (*top)(sg_handle, uint32_t, uint32_t, V, sg_node_out*, uint32_t*, size_t, size_t*, size_t*), uint32_t by,
                            uint32_t k, V min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index);
    // every trend row of the last flushed window through an indexed read (index NULL): the count first, then the rows
    template <class Row>
    long TrendRows(int (*read)(sg_handle, const uint32_t*, size_t, Row*, size_t, size_t*), std::vector<Row>* out) {
        if (!out || !read) return SG_EINVAL;
        std::lock_guard<std::mutex> fg(flush_mu_);
        size_t n = 0;
        int rc = read(h_, nullptr, 0, nullptr, 0, &n);
        if (rc != SG_OK) return rc;
        out->assign(n, Row{});
        if (n && (rc = read(h_, nullptr, 0, out->data(), n, &n)) != SG_OK) return rc;
        return (long)out->size();
    }

    datastore::DataStore* inner_;
    SgApi api_; sg_handle h_; EdgeSink* sink_;
    size_t max_edges_, batch_cap_;
    uint32_t max_known_; bool divert_;
    Shard shards_[kShards];                            // event batches, one per feeder-thread hash: appends do not serialise
    std::mutex id_mu_;                                 // ids_, uid_of_, kind_of_, refs_, the IP mirrors
    std::unordered_map<std::string, uint32_t> ids_;    // UID -> node id
    std::vector<std::string> uid_of_; std::vector<uint8_t> kind_of_; std::vector<uint32_t> refs_;
    std::unordered_map<uint32_t, uint32_t> pod_ip_id_, svc_ip_id_;   // ip -> id, what the engine's join tables hold
    std::vector<uint32_t> free_ids_, retired_;         // retired_: no IP left, reusable after the next FlushWindow
    size_t live_ids_ = 0;
    // the workload groups (under id_mu_): what the owners are is kept whether or not the groups are on
    bool groups_on_ = false; uint32_t max_groups_ = 0;
    uint64_t wl_entries_ = 0; size_t wl_van_rows_ = 0; // (flush_mu_) the workload baseline's capacity and the rows its vanished list holds, as the engine resolves a 0
    std::unordered_map<std::string, std::string> pod_owner_, rs_owner_;   // pod UID -> OwnerID; ReplicaSet UID -> its Deployment's UID
    std::unordered_map<std::string, uint32_t> gids_; std::vector<std::string> guid_of_;   // owner UID <-> group id, arrival order
    std::vector<uint32_t> node_group_;                 // node id -> the group the engine holds for it
    // the service binding (under id_mu_): what the Services and Endpoints are is kept whether or not the binding is on
    bool bind_on_ = false;
    std::unordered_map<std::string, std::string> svc_uid_;                  // "namespace/name" -> Service UID
    std::unordered_map<std::string, std::vector<std::string>> ep_pods_;     // "namespace/name" -> the pod UIDs behind it
    std::unordered_map<std::string, std::vector<std::string>> pod_eps_;     // pod UID -> the keys whose Endpoints name it
    std::vector<std::string> last_labels_; std::vector<uint32_t> last_obips_;   // of the last flushed window (flush_mu_)
    std::mutex pk_mu_;                                 // packer_ (labels, prepared statements, HPACK state), dto_labels_
    L7Packer packer_;
    std::unordered_map<std::string, uint32_t> dto_labels_;   // labels seen through the PersistRequest tap share the packer's id space
    size_t n_q_ = 2;                                   // quantiles per entity and side, as SetQuantiles set them last
    long LatencyRows(int (*read)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*), const uint32_t* index, size_t n_index,
                     size_t words, std::vector<uint32_t>* out_us);
    std::mutex flush_mu_;                              // one FlushWindow at a time; the selection below
    bool select_ = false; uint32_t sel_k_ = 0; float sel_min_ = 0;
    std::atomic<uint64_t> offered_{0}, batches_dropped_{0}, engine_errors_{0};
};

}  // namespace alaz
