#include "graph_ds.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>

namespace alaz {

bool SgApi::FromLibrary(void* dl, SgApi* o) {
    if (!dl || !o) return false;
#define SG_SYM(field, name) do { o->field = reinterpret_cast<decltype(o->field)>(dlsym(dl, name)); if (!o->field) return false; } while (0)
    SG_SYM(create, "sg_create"); SG_SYM(destroy, "sg_destroy"); SG_SYM(upsert_pod, "sg_upsert_pod"); SG_SYM(delete_pod, "sg_delete_pod");
    SG_SYM(upsert_service, "sg_upsert_service"); SG_SYM(delete_service, "sg_delete_service"); SG_SYM(set_label_count, "sg_set_label_count");
    SG_SYM(ingest, "sg_ingest"); SG_SYM(flush_window, "sg_flush_window"); SG_SYM(window_outbound_ips, "sg_window_outbound_ips");
    o->flush_window_view = reinterpret_cast<decltype(o->flush_window_view)>(dlsym(dl, "sg_flush_window_view"));   // optional
    o->flush_window_top = reinterpret_cast<decltype(o->flush_window_top)>(dlsym(dl, "sg_flush_window_top"));      // optional
    SG_SYM(last_error, "sg_last_error");
    o->set_groups = reinterpret_cast<decltype(o->set_groups)>(dlsym(dl, "sg_set_groups"));                        // optional (K14)
    o->group_assign = reinterpret_cast<decltype(o->group_assign)>(dlsym(dl, "sg_group_assign"));
    o->window_groups = reinterpret_cast<decltype(o->window_groups)>(dlsym(dl, "sg_window_groups"));
    o->set_group_trend = reinterpret_cast<decltype(o->set_group_trend)>(dlsym(dl, "sg_set_group_trend"));          // optional (K15)
    o->window_group_trend = reinterpret_cast<decltype(o->window_group_trend)>(dlsym(dl, "sg_window_group_trend"));
    o->set_group_vanished = reinterpret_cast<decltype(o->set_group_vanished)>(dlsym(dl, "sg_set_group_vanished"));
    o->window_group_vanished = reinterpret_cast<decltype(o->window_group_vanished)>(dlsym(dl, "sg_window_group_vanished"));
    o->window_groups_top = reinterpret_cast<decltype(o->window_groups_top)>(dlsym(dl, "sg_window_groups_top"));
    o->set_group_nodes = reinterpret_cast<decltype(o->set_group_nodes)>(dlsym(dl, "sg_set_group_nodes"));          // optional (K16)
    o->window_group_nodes = reinterpret_cast<decltype(o->window_group_nodes)>(dlsym(dl, "sg_window_group_nodes"));
    o->set_group_node_trend = reinterpret_cast<decltype(o->set_group_node_trend)>(dlsym(dl, "sg_set_group_node_trend"));
    o->window_group_node_trend = reinterpret_cast<decltype(o->window_group_node_trend)>(dlsym(dl, "sg_window_group_node_trend"));
    o->window_group_nodes_top = reinterpret_cast<decltype(o->window_group_nodes_top)>(dlsym(dl, "sg_window_group_nodes_top"));
    o->set_group_rank = reinterpret_cast<decltype(o->set_group_rank)>(dlsym(dl, "sg_set_group_rank"));             // optional (K17)
    o->window_group_rank_top = reinterpret_cast<decltype(o->window_group_rank_top)>(dlsym(dl, "sg_window_group_rank_top"));
    o->set_group_incidents = reinterpret_cast<decltype(o->set_group_incidents)>(dlsym(dl, "sg_set_group_incidents"));   // optional (K18)
    o->window_group_incidents = reinterpret_cast<decltype(o->window_group_incidents)>(dlsym(dl, "sg_window_group_incidents"));
    o->window_group_node_incident = reinterpret_cast<decltype(o->window_group_node_incident)>(dlsym(dl, "sg_window_group_node_incident"));
    o->set_group_tracks = reinterpret_cast<decltype(o->set_group_tracks)>(dlsym(dl, "sg_set_group_tracks"));   // optional (K19)
    o->window_group_incident_tracks = reinterpret_cast<decltype(o->window_group_incident_tracks)>(dlsym(dl, "sg_window_group_incident_tracks"));
    o->window_group_tracks_ended = reinterpret_cast<decltype(o->window_group_tracks_ended)>(dlsym(dl, "sg_window_group_tracks_ended"));
    o->set_group_impact = reinterpret_cast<decltype(o->set_group_impact)>(dlsym(dl, "sg_set_group_impact"));   // optional (K22)
    o->window_group_impact = reinterpret_cast<decltype(o->window_group_impact)>(dlsym(dl, "sg_window_group_impact"));
    o->set_quantiles = reinterpret_cast<decltype(o->set_quantiles)>(dlsym(dl, "sg_set_quantiles"));   // optional (K20)
    o->window_node_quantiles = reinterpret_cast<decltype(o->window_node_quantiles)>(dlsym(dl, "sg_window_node_quantiles"));
    o->window_group_quantiles = reinterpret_cast<decltype(o->window_group_quantiles)>(dlsym(dl, "sg_window_group_quantiles"));
    o->window_group_node_quantiles = reinterpret_cast<decltype(o->window_group_node_quantiles)>(dlsym(dl, "sg_window_group_node_quantiles"));
    o->set_quantile_trend = reinterpret_cast<decltype(o->set_quantile_trend)>(dlsym(dl, "sg_set_quantile_trend"));   // optional (K21)
    o->window_node_quantile_trend = reinterpret_cast<decltype(o->window_node_quantile_trend)>(dlsym(dl, "sg_window_node_quantile_trend"));
    o->window_group_quantile_trend = reinterpret_cast<decltype(o->window_group_quantile_trend)>(dlsym(dl, "sg_window_group_quantile_trend"));
    o->window_group_node_quantile_trend = reinterpret_cast<decltype(o->window_group_node_quantile_trend)>(dlsym(dl, "sg_window_group_node_quantile_trend"));
    o->window_group_nodes_top_tail = reinterpret_cast<decltype(o->window_group_nodes_top_tail)>(dlsym(dl, "sg_window_group_nodes_top_tail"));
    o->set_traffic_trend = reinterpret_cast<decltype(o->set_traffic_trend)>(dlsym(dl, "sg_set_traffic_trend"));   // optional (K23)
    o->window_group_nodes_top_traffic = reinterpret_cast<decltype(o->window_group_nodes_top_traffic)>(dlsym(dl, "sg_window_group_nodes_top_traffic"));
    o->set_slo = reinterpret_cast<decltype(o->set_slo)>(dlsym(dl, "sg_set_slo"));   // optional (K24)
    o->slo_assign = reinterpret_cast<decltype(o->slo_assign)>(dlsym(dl, "sg_slo_assign"));
    o->window_group_node_slo = reinterpret_cast<decltype(o->window_group_node_slo)>(dlsym(dl, "sg_window_group_node_slo"));
    o->window_group_nodes_top_slo = reinterpret_cast<decltype(o->window_group_nodes_top_slo)>(dlsym(dl, "sg_window_group_nodes_top_slo"));
    o->set_replicas = reinterpret_cast<decltype(o->set_replicas)>(dlsym(dl, "sg_set_replicas"));   // optional (K25)
    o->window_replicas = reinterpret_cast<decltype(o->window_replicas)>(dlsym(dl, "sg_window_replicas"));
    o->window_replicas_top = reinterpret_cast<decltype(o->window_replicas_top)>(dlsym(dl, "sg_window_replicas_top"));
#undef SG_SYM
    return true;
}

bool ParseIPv4(const std::string& s, uint32_t* out) {
    unsigned a, b, c, d; char tail;
    if (std::sscanf(s.c_str(), "%u.%u.%u.%u%c", &a, &b, &c, &d, &tail) != 4 || a > 255 || b > 255 || c > 255 || d > 255) return false;
    *out = (a << 24) | (b << 16) | (c << 8) | d;
    return true;
}
std::string FormatIPv4(uint32_t ip) {
    char buf[16];
    std::snprintf(buf, sizeof buf, "%u.%u.%u.%u", ip >> 24, (ip >> 16) & 255, (ip >> 8) & 255, ip & 255);
    return buf;
}

GraphDS::GraphDS(datastore::DataStore* inner, const SgApi& api, sg_handle h, EdgeSink* sink, size_t max_edges, size_t batch,
                 uint32_t max_known_nodes, bool divert_requests)
    : inner_(inner), api_(api), h_(h), sink_(sink), max_edges_(max_edges), batch_cap_(batch), max_known_(max_known_nodes), divert_(divert_requests) {
    for (Shard& s : shards_) s.batch.reserve(batch);
}
GraphDS::~GraphDS() = default;

uint32_t GraphDS::Intern(const std::string& uid, uint8_t kind) {
    auto it = ids_.find(uid);
    if (it != ids_.end()) { kind_of_[it->second] = kind; return it->second; }
    uint32_t id;
    if (!free_ids_.empty()) { id = free_ids_.back(); free_ids_.pop_back(); uid_of_[id] = uid; kind_of_[id] = kind; refs_[id] = 0; }
    else {
        if (uid_of_.size() >= max_known_) return kNoId;            // the engine's id space is full (sg_config.max_known_nodes)
        id = (uint32_t)uid_of_.size();
        uid_of_.push_back(uid); kind_of_.push_back(kind); refs_.push_back(0);
    }
    ids_.emplace(uid, id);
    live_ids_++;
    return id;
}
void GraphDS::UnbindIP(std::unordered_map<uint32_t, uint32_t>& m, uint32_t ip) {
    auto it = m.find(ip);
    if (it == m.end()) return;
    const uint32_t id = it->second;
    m.erase(it);
    if (--refs_[id] == 0) retired_.push_back(id);                  // no IP names it any more; the open window may still do
}
void GraphDS::BindIP(std::unordered_map<uint32_t, uint32_t>& m, uint32_t ip, uint32_t id) {
    auto it = m.find(ip);
    if (it != m.end() && it->second == id) return;
    refs_[id]++;                                                     // before the unbind: re-binding an id's only IP must not retire it
    if (it != m.end()) { const uint32_t old = it->second; it->second = id; if (--refs_[old] == 0) retired_.push_back(old); }
    else m.emplace(ip, id);
}

// ---- the workload groups (id_mu_ held) ----
uint32_t GraphDS::GroupOfOwner(const std::string& owner) {
    if (owner.empty()) return kNoId;
    auto rs = rs_owner_.find(owner);
    const std::string& top = rs != rs_owner_.end() && !rs->second.empty() ? rs->second : owner;   // ReplicaSet -> its Deployment
    auto it = gids_.find(top);
    if (it != gids_.end()) return it->second;
    if (guid_of_.size() >= max_groups_) { engine_errors_++; return kNoId; }
    const uint32_t g = (uint32_t)guid_of_.size();
    guid_of_.push_back(top); gids_.emplace(top, g);
    return g;
}
void GraphDS::AssignGroup(uint32_t id, uint32_t group) {
    if (id >= node_group_.size()) node_group_.resize(id + 1, kNoId);
    if (node_group_[id] == group) return;
    if (api_.group_assign(h_, &id, &group, 1) == SG_OK) node_group_[id] = group; else engine_errors_++;
}
int GraphDS::SetWorkloadGroups(uint32_t max_groups) {
    if (!api_.set_groups || !api_.group_assign) return SG_EINVAL;
    std::lock_guard<std::mutex> g(id_mu_);
    sg_group_params p{}; p.struct_size = sizeof p; p.max_groups = max_groups;
    const int rc = api_.set_groups(h_, &p);
    if (rc != SG_OK) return rc;
    groups_on_ = true; max_groups_ = max_groups ? max_groups : max_known_;
    gids_.clear(); guid_of_.clear(); node_group_.clear();             // the engine's map starts over: the pods known so far, in id order
    for (uint32_t id = 0; id < uid_of_.size(); id++) {
        if (kind_of_[id] != SG_NODE_POD || uid_of_[id].empty()) continue;
        auto po = pod_owner_.find(uid_of_[id]);
        if (po != pod_owner_.end()) AssignGroup(id, GroupOfOwner(po->second));
    }
    if (bind_on_) BindAllServices();
    return SG_OK;
}
// ---- the service binding (id_mu_ held) ----
static std::string ServiceKey(const std::string& ns, const std::string& name) { return ns + "/" + name; }
void GraphDS::BindService(const std::string& key) {
    auto sv = svc_uid_.find(key);
    if (sv == svc_uid_.end()) return;
    auto sid = ids_.find(sv->second);
    if (sid == ids_.end() || kind_of_[sid->second] != SG_NODE_SERVICE) return;   // (no ClusterIP here: no node id to assign)
    uint32_t group = kNoId;
    bool any = false, one = true;
    auto ep = ep_pods_.find(key);
    if (bind_on_ && groups_on_ && ep != ep_pods_.end())
        for (const std::string& pod : ep->second) {
            auto p = ids_.find(pod);
            if (p == ids_.end() || kind_of_[p->second] != SG_NODE_POD || refs_[p->second] == 0) continue;   // a pod the store does not know
            const uint32_t g = p->second < node_group_.size() ? node_group_[p->second] : kNoId;
            if (g == kNoId || (any && g != group)) one = false;       // an ungrouped pod among them, or two workloads behind it
            group = g; any = true;
        }
    const uint32_t want = any && one ? group : kNoId;
    if (want == kNoId && sid->second >= node_group_.size()) return;    // (never assigned: nothing to take back)
    AssignGroup(sid->second, want);
}
void GraphDS::BindServicesOfPod(const std::string& pod_uid) {
    auto it = pod_eps_.find(pod_uid);
    if (it == pod_eps_.end()) return;
    for (const std::string& key : it->second) BindService(key);
}
void GraphDS::BindAllServices() {
    for (const auto& kv : svc_uid_) BindService(kv.first);
}
int GraphDS::SetServiceBinding(bool on) {
    if (!api_.group_assign) return SG_EINVAL;
    std::lock_guard<std::mutex> g(id_mu_);
    if (!groups_on_) return SG_ESTATE;
    bind_on_ = on;
    BindAllServices();
    return SG_OK;
}
int GraphDS::PersistEndpoints(const datastore::Endpoints& e, const std::string& et) {
    const bool up = et == datastore::ADD || et == datastore::UPDATE;
    if (up || et == datastore::DELETE_) {
        std::lock_guard<std::mutex> g(id_mu_);
        const std::string key = ServiceKey(e.Namespace, e.Name);
        auto old = ep_pods_.find(key);
        if (old != ep_pods_.end()) {
            for (const std::string& pod : old->second) {
                auto pe = pod_eps_.find(pod);
                if (pe == pod_eps_.end()) continue;
                pe->second.erase(std::remove(pe->second.begin(), pe->second.end(), key), pe->second.end());
                if (pe->second.empty()) pod_eps_.erase(pe);
            }
            ep_pods_.erase(old);
        }
        if (up) {
            std::vector<std::string>& pods = ep_pods_[key];
            for (const datastore::Address& a : e.Addresses)
                for (const datastore::AddressIP& ip : a.IPs)      // (TargetRef's kind and UID, aggregator/persist.go:247-267)
                    if (ip.Type == "Pod" && !ip.ID.empty() && std::find(pods.begin(), pods.end(), ip.ID) == pods.end()) pods.push_back(ip.ID);
            for (const std::string& pod : pods) pod_eps_[pod].push_back(key);
        }
        BindService(key);
    }
    return inner_->PersistEndpoints(e, et);
}
int GraphDS::PersistReplicaSet(const datastore::ReplicaSet& rs, const std::string& et) {
    if (et == datastore::ADD || et == datastore::UPDATE) {
        std::lock_guard<std::mutex> g(id_mu_);
        std::string& dep = rs_owner_[rs.UID];
        if (dep != rs.OwnerID) {
            dep = rs.OwnerID;
            if (groups_on_)                                             // its pods came first: they move to the Deployment's group
                for (const auto& po : pod_owner_) {
                    if (po.second != rs.UID) continue;
                    auto it = ids_.find(po.first);
                    if (it != ids_.end()) { AssignGroup(it->second, GroupOfOwner(rs.UID)); BindServicesOfPod(po.first); }
                }
        }
    } else if (et == datastore::DELETE_) { std::lock_guard<std::mutex> g(id_mu_); rs_owner_.erase(rs.UID); }   // (its pods keep their group)
    return inner_->PersistReplicaSet(rs, et);
}
long GraphDS::WorkloadEdges(std::vector<WorkloadEdge>* out) {
    if (!out || !api_.window_groups) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_groups(h_, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    std::vector<sg_group_edge> ge(n);
    if (n && (rc = api_.window_groups(h_, ge.data(), n, &n)) != SG_OK) return rc;
    out->assign(ge.size(), WorkloadEdge{});
    std::lock_guard<std::mutex> g(id_mu_);
    for (size_t i = 0; i < ge.size(); i++) NameWorkloadEdge(ge[i], &(*out)[i]);
    return (long)ge.size();
}
void GraphDS::NameRef(uint32_t ref, std::string* type, std::string* uid) const {
    const uint32_t t = SG_REF_TYPE(ref), v = SG_REF_VALUE(ref);
    if (t == SG_REF_GROUP && v < guid_of_.size()) { *type = "workload"; *uid = guid_of_[v]; }
    else if (t == SG_REF_KNOWN && v < uid_of_.size()) { *type = kind_of_[v] == SG_NODE_SERVICE ? "service" : "pod"; *uid = uid_of_[v]; }
    else if (t == SG_REF_LABEL && v < last_labels_.size()) { *type = "outbound"; *uid = last_labels_[v]; }
    else if (t == SG_REF_OBIP && v < last_obips_.size()) { *type = "outbound"; *uid = FormatIPv4(last_obips_[v]); }
    else { *type = "unknown"; uid->clear(); }
}
void GraphDS::NameWorkloadEdge(const sg_group_edge& r, WorkloadEdge* out) const {
    WorkloadEdge& o = *out;
    NameRef(r.from_ref, &o.FromType, &o.FromUID); NameRef(r.to_ref, &o.ToType, &o.ToUID);
    o.Count = r.count; o.ErrCount = r.err_count; o.SumNs = r.sum_ns; o.SumSqUs = r.sumsq_us; o.MaxNs = r.max_ns; o.ScoreQ32 = r.score_q32;
    o.Edges = r.edges; o.FromNodes = r.from_nodes; o.Alive = r.alive; o.WorstRow = r.worst_row; o.ScoreMax = r.score_max;
}

// ---- the workload baselines (K15) ----
int GraphDS::SetWorkloadTrend(const sg_trend_params& p) {
    if (!api_.set_group_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);                        // (not beside a FlushWindow: the engine refuses it while a flush is open)
    const int rc = api_.set_group_trend(h_, &p);
    if (rc == SG_OK) wl_entries_ = p.max_entries ? p.max_entries : std::min<uint64_t>(1ull << 31, 2 * std::max<uint64_t>(max_edges_, 1));
    return rc;
}
int GraphDS::SetWorkloadVanished(const sg_vanished_params& p) {
    if (!api_.set_group_vanished) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    const int rc = api_.set_group_vanished(h_, &p);
    if (rc == SG_OK) wl_van_rows_ = p.max_rows ? p.max_rows : (size_t)std::min<uint64_t>(65536, wl_entries_);   // (sg_vanished_params' default)
    return rc;
}
long GraphDS::WorkloadTrends(std::vector<sg_edge_trend>* out) {
    if (!out || !api_.window_group_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_trend(h_, nullptr, 0, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    out->assign(n, sg_edge_trend{});
    if (n && (rc = api_.window_group_trend(h_, nullptr, 0, out->data(), n, &n)) != SG_OK) return rc;
    return (long)out->size();
}
long GraphDS::WorkloadTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadEdge>* out, std::vector<uint32_t>* index) {
    if (!out || !api_.window_groups_top) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t sel = 0, total = 0;
    std::vector<sg_group_edge> ge;
    std::vector<uint32_t> idx;
    if (k) { ge.resize(k); idx.resize(k); }                          // at most k are selected; k = 0: the count first
    int rc = api_.window_groups_top(h_, by, k, min_value, ge.data(), idx.data(), ge.size(), &sel, &total);
    if (rc != SG_OK) return rc;
    if (!k && sel) {
        ge.resize(sel); idx.resize(sel);
        if ((rc = api_.window_groups_top(h_, by, 0, min_value, ge.data(), idx.data(), ge.size(), &sel, &total)) != SG_OK) return rc;
    }
    const size_t m = std::min(sel, ge.size());
    ge.resize(m); idx.resize(m);
    out->assign(m, WorkloadEdge{});
    {
        std::lock_guard<std::mutex> g(id_mu_);
        for (size_t i = 0; i < m; i++) NameWorkloadEdge(ge[i], &(*out)[i]);
    }
    if (index) *index = std::move(idx);
    return (long)m;
}
long GraphDS::WorkloadVanished(std::vector<VanishedWorkload>* out) {
    if (!out || !api_.window_group_vanished) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_vanished(h_, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    std::vector<sg_edge_vanished> v(std::min(n, wl_van_rows_));        // n counts every vanished entry; the list holds at most max_rows of them
    if (!v.empty() && (rc = api_.window_group_vanished(h_, v.data(), v.size(), &n)) != SG_OK) return rc;
    out->clear();
    std::lock_guard<std::mutex> g(id_mu_);
    auto uid = [&](uint64_t key) { return (key >> 32) == 0 && key < guid_of_.size() ? guid_of_[(size_t)key] : std::string(); };
    for (const sg_edge_vanished& r : v) {
        VanishedWorkload o;
        o.FromKey = r.from_key; o.ToKey = r.to_key; o.FromUID = uid(r.from_key); o.ToUID = uid(r.to_key);
        o.LatMean = r.lat_mean; o.LatDev = r.lat_dev; o.ErrMean = r.err_mean; o.ErrDev = r.err_dev; o.N = r.n; o.Last = r.last; o.Row = r.row;
        out->push_back(o);
    }
    return (long)out->size();
}

// ---- the workload rows (K16) ----
int GraphDS::SetWorkloadNodes(bool on) {
    if (!api_.set_group_nodes) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);                        // (not beside a FlushWindow: the engine refuses it while a flush is open)
    return api_.set_group_nodes(h_, on ? 1 : 0);
}
int GraphDS::SetWorkloadNodeTrend(const sg_trend_params& p) {
    if (!api_.set_group_node_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_group_node_trend(h_, &p);
}
void GraphDS::NameWorkloadNodes(const std::vector<sg_node_out>& rows, std::vector<WorkloadNode>* out) {
    out->assign(rows.size(), WorkloadNode{});
    std::lock_guard<std::mutex> g(id_mu_);
    for (size_t i = 0; i < rows.size(); i++) { NameRef(rows[i].ref, &(*out)[i].Type, &(*out)[i].UID); (*out)[i].Row = rows[i]; }
}
long GraphDS::WorkloadNodes(std::vector<WorkloadNode>* out) {
    if (!out || !api_.window_group_nodes) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_nodes(h_, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    std::vector<sg_node_out> rows(n);
    if (n && (rc = api_.window_group_nodes(h_, rows.data(), n, &n)) != SG_OK) return rc;
    NameWorkloadNodes(rows, out);
    return (long)rows.size();
}
long GraphDS::WorkloadNodeTrends(std::vector<sg_node_trend>* out) {
    if (!out || !api_.window_group_node_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_node_trend(h_, nullptr, 0, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    out->assign(n, sg_node_trend{});
    if (n && (rc = api_.window_group_node_trend(h_, nullptr, 0, out->data(), n, &n)) != SG_OK) return rc;
    return (long)out->size();
}
long GraphDS::WorkloadNodesTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index) {
    return WorkloadNodesTopBy(api_.window_group_nodes_top, by, k, min_value, out, index);
}
template <class V>
long GraphDS::WorkloadNodesTopBy(int (*top)(sg_handle, uint32_t, uint32_t, V, sg_node_out*, uint32_t*, size_t, size_t*, size_t*), uint32_t by,
                                 uint32_t k, V min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index) {
    if (!out || !top) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t sel = 0, total = 0;
    std::vector<sg_node_out> rows;
    std::vector<uint32_t> idx;
    if (k) { rows.resize(k); idx.resize(k); }                        // at most k are selected; k = 0: the count first
    int rc = top(h_, by, k, min_value, rows.data(), idx.data(), rows.size(), &sel, &total);
    if (rc != SG_OK) return rc;
    if (!k && sel) {
        rows.resize(sel); idx.resize(sel);
        if ((rc = top(h_, by, 0, min_value, rows.data(), idx.data(), rows.size(), &sel, &total)) != SG_OK) return rc;
    }
    const size_t m = std::min(sel, rows.size());
    rows.resize(m); idx.resize(m);
    NameWorkloadNodes(rows, out);
    if (index) *index = std::move(idx);
    return (long)m;
}

// ---- the workload ranking (K17) ----
int GraphDS::SetWorkloadRank(const sg_rank_params* p) {
    if (!api_.set_group_rank) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_group_rank(h_, p);
}
long GraphDS::WorkloadCulprits(uint32_t k, float min_share, std::vector<WorkloadCulprit>* out, std::vector<uint32_t>* index) {
    if (!out || !api_.window_group_rank_top) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t sel = 0, total = 0;
    std::vector<sg_node_out> rows;
    std::vector<sg_node_rank> ranks;
    std::vector<uint32_t> idx;
    if (k) { rows.resize(k); ranks.resize(k); idx.resize(k); }       // at most k are selected; k = 0: the count first
    int rc = api_.window_group_rank_top(h_, k, min_share, rows.data(), ranks.data(), idx.data(), rows.size(), &sel, &total);
    if (rc != SG_OK) return rc;
    if (!k && sel) {
        rows.resize(sel); ranks.resize(sel); idx.resize(sel);
        if ((rc = api_.window_group_rank_top(h_, 0, min_share, rows.data(), ranks.data(), idx.data(), rows.size(), &sel, &total)) != SG_OK) return rc;
    }
    const size_t m = std::min(sel, rows.size());
    rows.resize(m); idx.resize(m);
    std::vector<WorkloadNode> named;
    NameWorkloadNodes(rows, &named);
    out->assign(m, WorkloadCulprit{});
    for (size_t i = 0; i < m; i++) { (*out)[i].Node = std::move(named[i]); (*out)[i].Rank = ranks[i]; }
    if (index) *index = std::move(idx);
    return (long)m;
}

// ---- the workload incidents (K18) ----
int GraphDS::SetWorkloadIncidents(const sg_incident_params* p) {
    if (!api_.set_group_incidents) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_group_incidents(h_, p);
}
long GraphDS::WorkloadIncidents(std::vector<sg_incident_out>* out, std::vector<uint32_t>* node_incident) {
    if (!out || !api_.window_group_incidents || (node_incident && !api_.window_group_node_incident)) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_incidents(h_, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    out->assign(n, sg_incident_out{});
    if (n && (rc = api_.window_group_incidents(h_, out->data(), n, &n)) != SG_OK) return rc;
    if (node_incident) {
        size_t m = 0;
        if ((rc = api_.window_group_node_incident(h_, nullptr, 0, nullptr, 0, &m)) != SG_OK) return rc;
        node_incident->assign(m, SG_NO_INCIDENT);
        if (m && (rc = api_.window_group_node_incident(h_, nullptr, 0, node_incident->data(), m, &m)) != SG_OK) return rc;
    }
    return (long)out->size();
}

// ---- the workload tracks (K19) ----
int GraphDS::SetWorkloadTracks(const sg_track_params* p) {
    if (!api_.set_group_tracks) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_group_tracks(h_, p);
}
// a counted list of the last flushed window: the count first, then the rows
template <class Row>
static long counted_rows(sg_handle h, int (*read)(sg_handle, Row*, size_t, size_t*), std::vector<Row>* out) {
    size_t n = 0;
    int rc = read(h, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    out->assign(n, Row{});
    if (n && (rc = read(h, out->data(), n, &n)) != SG_OK) return rc;
    return (long)out->size();
}
long GraphDS::WorkloadIncidentTracks(std::vector<sg_incident_track>* out) {
    if (!out || !api_.window_group_incident_tracks) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return counted_rows(h_, api_.window_group_incident_tracks, out);
}
long GraphDS::WorkloadTracksEnded(std::vector<sg_track_entry>* out) {
    if (!out || !api_.window_group_tracks_ended) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return counted_rows(h_, api_.window_group_tracks_ended, out);
}

// ---- the workload impact (K22) ----
int GraphDS::SetWorkloadImpact(uint32_t max_incidents, uint32_t max_hops) {
    if (!api_.set_group_impact) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_group_impact(h_, max_incidents, max_hops);
}
long GraphDS::WorkloadImpact(std::vector<sg_incident_out>* incidents, std::vector<uint64_t>* impact) {
    if (!incidents || !impact || !api_.window_group_incidents || !api_.window_group_impact) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    const long rc = counted_rows(h_, api_.window_group_incidents, incidents);
    if (rc < 0) return rc;
    size_t n = 0;
    int r = api_.window_group_impact(h_, nullptr, 0, &n);
    if (r != SG_OK) return r;
    impact->assign(n * SG_IMPACT_WORDS, 0);
    if (n && (r = api_.window_group_impact(h_, impact->data(), n, &n)) != SG_OK) return r;
    return (long)n;
}

// ---- the latency percentiles (K20) ----
int GraphDS::SetQuantiles(uint32_t spaces, const uint32_t* permille, size_t n_q) {
    if (!api_.set_quantiles) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    const int rc = api_.set_quantiles(h_, spaces, permille, n_q);
    if (rc == SG_OK) n_q_ = n_q ? n_q : 2;
    return rc;
}
// ---- the tail baselines (K21) ----
int GraphDS::SetTailTrend(uint32_t spaces, uint32_t permille, const sg_trend_params* p) {
    if (!api_.set_quantile_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_quantile_trend(h_, spaces, permille, p);
}
long GraphDS::NodeTailTrends(std::vector<sg_node_trend>* out) { return TrendRows(api_.window_node_quantile_trend, out); }
long GraphDS::WorkloadEdgeTailTrends(std::vector<sg_edge_trend>* out) { return TrendRows(api_.window_group_quantile_trend, out); }
long GraphDS::WorkloadTailTrends(std::vector<sg_node_trend>* out) { return TrendRows(api_.window_group_node_quantile_trend, out); }
long GraphDS::WorkloadTailTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index) {
    return WorkloadNodesTopBy(api_.window_group_nodes_top_tail, by, k, min_value, out, index);
}
// ---- the traffic baselines (K23) ----
int GraphDS::SetTrafficTrend(uint32_t spaces, const sg_traffic_params* p) {
    if (!api_.set_traffic_trend) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_traffic_trend(h_, spaces, p);
}
long GraphDS::WorkloadTrafficTop(uint32_t by, uint32_t k, float min_value, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index) {
    return WorkloadNodesTopBy(api_.window_group_nodes_top_traffic, by, k, min_value, out, index);
}
// ---- the replica outliers (K25) ----
int GraphDS::SetReplicaOutliers(const sg_replica_params* p) {
    if (!api_.set_replicas) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_replicas(h_, p);
}
long GraphDS::WorkloadReplicaOutliers(uint32_t by, uint32_t k, uint32_t min_value, std::vector<ReplicaOutlier>* out) {
    if (!out || !api_.window_replicas_top || !api_.window_replicas || !api_.window_group_nodes) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t sel = 0, total = 0;
    std::vector<sg_node_out> rows;
    std::vector<uint32_t> idx;
    if (k) { rows.resize(k); idx.resize(k); }                        // at most k are selected; k = 0: the count first
    int rc = api_.window_replicas_top(h_, by, k, min_value, rows.data(), idx.data(), rows.size(), &sel, &total);
    if (rc != SG_OK) return rc;
    if (!k && sel) {
        rows.resize(sel); idx.resize(sel);
        if ((rc = api_.window_replicas_top(h_, by, 0, min_value, rows.data(), idx.data(), rows.size(), &sel, &total)) != SG_OK) return rc;
    }
    const size_t m = std::min(sel, rows.size());
    rows.resize(m); idx.resize(m);
    out->assign(m, ReplicaOutlier{});
    if (!m) return 0;
    std::vector<uint32_t> pods(m * SG_REPLICA_WORDS);
    size_t n = 0;
    if ((rc = api_.window_replicas(h_, idx.data(), m, pods.data(), m, &n)) != SG_OK) return rc;
    if ((rc = api_.window_group_nodes(h_, nullptr, 0, &n)) != SG_OK) return rc;
    std::vector<sg_node_out> wl(n);
    if (n && (rc = api_.window_group_nodes(h_, wl.data(), n, &n)) != SG_OK) return rc;
    const uint32_t* side0 = pods.data() + 2 + ((by & SG_RSEL_OUT) ? 5 : 0);
    std::lock_guard<std::mutex> g(id_mu_);
    for (size_t i = 0; i < m; i++) {
        ReplicaOutlier& o = (*out)[i];
        const uint32_t* r = pods.data() + i * SG_REPLICA_WORDS;
        const uint32_t* s = side0 + i * SG_REPLICA_WORDS;
        std::string type;
        NameRef(rows[i].ref, &type, &o.PodUID);
        o.NodeIndex = idx[i]; o.WorkloadIndex = r[0]; o.Flags = r[1];
        if (r[0] < wl.size()) NameRef(wl[r[0]].ref, &type, &o.Workload);
        o.ErrExcessQ20 = (int32_t)s[0]; o.LatRatioQ10 = s[1]; o.ShareQ10 = s[2]; o.TailPod = s[3] & 255u; o.TailPeers = s[3] >> 8 & 255u; o.Replicas = s[4];
    }
    return (long)m;
}
// ---- the SLO burn rates (K24) ----
int GraphDS::SetSLO(uint32_t spaces, const sg_slo_params* p) {
    if (!api_.set_slo) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    return api_.set_slo(h_, spaces, p);
}
int GraphDS::SetWorkloadSLO(const std::string& workload, uint32_t objective) {
    if (!api_.slo_assign) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    uint32_t ref;
    {
        std::lock_guard<std::mutex> g(id_mu_);
        auto it = gids_.find(workload);
        if (it == gids_.end()) return SG_EINVAL;
        ref = SG_MAKE_REF(SG_REF_GROUP, it->second);
    }
    return api_.slo_assign(h_, SG_Q_GROUP_NODES, &ref, &objective, 1);
}
long GraphDS::WorkloadSLO(std::vector<uint64_t>* out) {
    if (!out || !api_.window_group_node_slo) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = 0;
    int rc = api_.window_group_node_slo(h_, nullptr, 0, nullptr, 0, &n);
    if (rc != SG_OK) return rc;
    out->assign(n * SG_SLO_WORDS, 0ull);
    if (n && (rc = api_.window_group_node_slo(h_, nullptr, 0, out->data(), n, &n)) != SG_OK) return rc;
    return (long)n;
}
long GraphDS::WorkloadSLOTop(uint32_t by, uint32_t k, uint32_t min_value_q10, std::vector<WorkloadNode>* out, std::vector<uint32_t>* index) {
    return WorkloadNodesTopBy(api_.window_group_nodes_top_slo, by, k, min_value_q10, out, index);
}

// the quantiles of the last flushed window, `words` u32 an entity: the count first (no index), then the rows
long GraphDS::LatencyRows(int (*read)(sg_handle, const uint32_t*, size_t, uint32_t*, size_t, size_t*), const uint32_t* index, size_t n_index,
                          size_t words, std::vector<uint32_t>* out_us) {
    if (!out_us || !read) return SG_EINVAL;
    std::lock_guard<std::mutex> fg(flush_mu_);
    size_t n = index ? n_index : 0;
    int rc;
    if (!index && (rc = read(h_, nullptr, 0, nullptr, 0, &n)) != SG_OK) return rc;
    out_us->assign(n * words, 0u);
    if (n && (rc = read(h_, index, n_index, out_us->data(), n, &n)) != SG_OK) return rc;
    return (long)n;
}
long GraphDS::NodeLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us) {
    return LatencyRows(api_.window_node_quantiles, index, n_index, 2 * n_q_, out_us);
}
long GraphDS::WorkloadEdgeLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us) {
    return LatencyRows(api_.window_group_quantiles, index, n_index, n_q_, out_us);
}
long GraphDS::WorkloadLatency(const uint32_t* index, size_t n_index, std::vector<uint32_t>* out_us) {
    return LatencyRows(api_.window_group_node_quantiles, index, n_index, 2 * n_q_, out_us);
}

// processPod keeps PodIPToPodUid (aggregator/persist.go:55-71); pods without an IP never reach the
// datastore (persist.go:37-40), an empty IP here is ignored for the same reason.
int GraphDS::PersistPod(const datastore::Pod& pod, const std::string& et) {
    uint32_t ip; int erc = SG_OK;
    if (!pod.IP.empty() && ParseIPv4(pod.IP, &ip)) {
        const bool up = et == datastore::ADD || et == datastore::UPDATE;
        if (up || et == datastore::DELETE_) {
            std::lock_guard<std::mutex> g(id_mu_);
            if (up) {
                const uint32_t id = Intern(pod.UID, SG_NODE_POD);
                erc = id == kNoId ? SG_ENOSPC : api_.upsert_pod(h_, ip, id);
                if (erc == SG_OK) {
                    BindIP(pod_ip_id_, ip, id);
                    pod_owner_[pod.UID] = pod.OwnerID;
                    if (groups_on_) AssignGroup(id, GroupOfOwner(pod.OwnerID));
                    BindServicesOfPod(pod.UID);
                }
            } else { api_.delete_pod(h_, ip); UnbindIP(pod_ip_id_, ip); BindServicesOfPod(pod.UID); }     // (a DELETE never creates an id; its group goes with the id, in FlushWindow)
        }
        if (erc == SG_OK && (up || et == datastore::DELETE_)) { std::lock_guard<std::mutex> g(pk_mu_); packer_.SetPodIP(ip, up); }
        if (erc != SG_OK) engine_errors_++;
    }
    const int rc = inner_->PersistPod(pod, et);
    return rc != 0 ? rc : erc;
}

// processSvc keys ServiceIPToServiceUid on Spec.ClusterIP (persist.go:114-130); the DTO carries it as
// ClusterIPs[0] (ClusterIP itself is never filled in, persist.go:105-112).
int GraphDS::PersistService(const datastore::Service& svc, const std::string& et) {
    const std::string& ips = !svc.ClusterIPs.empty() ? svc.ClusterIPs[0] : svc.ClusterIP;
    uint32_t ip; int erc = SG_OK;
    if (ParseIPv4(ips, &ip)) {
        const bool up = et == datastore::ADD || et == datastore::UPDATE;
        if (up || et == datastore::DELETE_) {
            std::lock_guard<std::mutex> g(id_mu_);
            if (up) {
                const uint32_t id = Intern(svc.UID, SG_NODE_SERVICE);
                erc = id == kNoId ? SG_ENOSPC : api_.upsert_service(h_, ip, id);
                if (erc == SG_OK) {
                    BindIP(svc_ip_id_, ip, id);
                    if (!svc.Name.empty()) { const std::string key = svc.Namespace + "/" + svc.Name; svc_uid_[key] = svc.UID; BindService(key); }
                }
            } else {
                if (!svc.Name.empty()) {                             // forget the entry: a bound Service leaves its group first
                    const std::string key = svc.Namespace + "/" + svc.Name;
                    auto sv = svc_uid_.find(key);
                    if (sv != svc_uid_.end()) {
                        auto sid = ids_.find(sv->second);
                        if (sid != ids_.end() && sid->second < node_group_.size()) AssignGroup(sid->second, kNoId);
                        svc_uid_.erase(sv);
                    }
                }
                api_.delete_service(h_, ip); UnbindIP(svc_ip_id_, ip);
            }
        }
        if (erc == SG_OK && (up || et == datastore::DELETE_)) { std::lock_guard<std::mutex> g(pk_mu_); packer_.SetServiceIP(ip, up); }
        if (erc != SG_OK) engine_errors_++;
    }
    const int rc = inner_->PersistService(svc, et);
    return rc != 0 ? rc : erc;
}

int GraphDS::FlushShard(Shard& s) {
    if (s.batch.empty()) return SG_OK;
    const int rc = api_.ingest(h_, s.batch.data(), s.batch.size());   // copies; the engine has its own lock
    if (rc == SG_EAGAIN) batches_dropped_++;          // never block the aggregator (the reference would: backend.go:844)
    s.batch.clear();
    return rc == SG_EAGAIN ? SG_OK : rc;
}

// events of one caller go to the shard its thread hashes to: goroutines on different OS threads do not meet here
int GraphDS::Append(const sg_event* ev, size_t n) {
    if (n == 0) return SG_OK;
    Shard& s = shards_[std::hash<std::thread::id>()(std::this_thread::get_id()) % kShards];
    std::lock_guard<std::mutex> g(s.mu);
    int rc = SG_OK;
    for (size_t i = 0; i < n; i++) {
        s.batch.push_back(ev[i]);
        if (s.batch.size() >= batch_cap_) { const int r2 = FlushShard(s); if (r2 != SG_OK) rc = r2; }
    }
    offered_ += n;
    return rc;
}

static uint8_t ProtocolId(const std::string& p, bool* tls) {
    if (p == "HTTPS") { *tls = true; return SG_PROTO_HTTP; }     // rewrite of data.go:1240-1242 undone
    static const char* names[] = {"UNKNOWN", "HTTP", "AMQP", "POSTGRES", "HTTP2", "REDIS", "KAFKA", "MYSQL", "MONGO"};
    for (uint8_t i = 0; i <= 8; i++) if (p == names[i]) return i;
    return SG_PROTO_UNKNOWN;
}

// The datastore-boundary tap.  The DTO is only read during the call (cgo rule; backend.go:824-839).
int GraphDS::PersistAliveConnection(const datastore::AliveConnection* c) {
    if (!c) return SG_EINVAL;
    sg_event ev; std::memset(&ev, 0, sizeof ev);
    if (ParseIPv4(c->FromIP, &ev.saddr) && ParseIPv4(c->ToIP, &ev.daddr)) {
        ev.flags = SG_EV_ALIVE;
        Append(&ev, 1);
    }
    return inner_->PersistAliveConnection(c);
}

int GraphDS::PersistRequest(const datastore::Request* r) {
    if (!r) return SG_EINVAL;
    sg_event ev; std::memset(&ev, 0, sizeof ev);
    bool tls = r->Tls;
    ev.protocol = ProtocolId(r->Protocol, &tls);
    // ReverseDirection() was applied for AMQP DELIVER / Redis PUSHED_EVENT (data.go:1110-1112,1151-1153): undo it,
    // K1 re-applies it after its own join
    const bool rev = (ev.protocol == SG_PROTO_AMQP && r->Method == "DELIVER") || (ev.protocol == SG_PROTO_REDIS && r->Method == "PUSHED_EVENT");
    const std::string& sip = rev ? r->ToIP : r->FromIP; const std::string& dip = rev ? r->FromIP : r->ToIP;
    const std::string& dtype = rev ? r->FromType : r->ToType; const std::string& duid = rev ? r->FromUID : r->ToUID;
    if (!ParseIPv4(sip, &ev.saddr) || !ParseIPv4(dip, &ev.daddr)) return SG_OK;   // not IPv4: nothing the join could do
    ev.status = (uint16_t)(r->StatusCode > 0xFFFFu ? 0xFFFFu : r->StatusCode);
    ev.flags = (tls ? SG_EV_TLS : 0) | (rev ? SG_EV_REVERSE : 0);
    ev.duration_ns = r->Latency;
    ev.write_time_ns = (uint64_t)r->StartTime * 1000000ull;       // already wall-clock ms; the engine clock is (0, 0) for this tap
    if (dtype == "outbound" && duid != dip) {                     // named by Host header (or reverse DNS): a label
        std::lock_guard<std::mutex> g(pk_mu_);
        auto it = dto_labels_.find(duid);
        if (it == dto_labels_.end()) {
            std::vector<sg_event> tmp;                            // intern through the packer so both taps share one id space
            l7_req::L7Event fake; fake.ProtocolId = SG_PROTO_HTTP; fake.Daddr = ev.daddr;
            const std::string pl = "GET / HTTP/1.1\r\nHost: " + duid + "\r\n";
            fake.PayloadSize = (uint32_t)std::min(pl.size(), l7_req::kMaxPayload); std::memcpy(fake.Payload, pl.data(), fake.PayloadSize);
            if (!packer_.IsKnownIP(ev.daddr)) { packer_.Pack(fake, 1, &tmp); if (!tmp.empty()) it = dto_labels_.emplace(duid, tmp[0].host_label).first; }
        }
        if (it != dto_labels_.end()) ev.host_label = it->second;
    }
    const int rc = Append(&ev, 1);
    if (!divert_) { const int r2 = inner_->PersistRequest(r); if (r2 != 0) return r2; }   // additive by default
    return rc;
}

int GraphDS::PersistKafkaEvent(const datastore::KafkaEvent* k) {
    if (!k) return SG_EINVAL;
    sg_event ev; std::memset(&ev, 0, sizeof ev);
    if (!ParseIPv4(k->FromIP, &ev.saddr) || !ParseIPv4(k->ToIP, &ev.daddr)) return SG_OK;
    ev.protocol = SG_PROTO_KAFKA; ev.status = 1;
    ev.flags = (k->Tls ? SG_EV_TLS : 0) | (k->Type == "CONSUME" ? SG_EV_CONSUME : 0);
    ev.duration_ns = k->Latency; ev.write_time_ns = (uint64_t)k->StartTime * 1000000ull;
    const int rc = Append(&ev, 1);
    if (!divert_) { const int r2 = inner_->PersistKafkaEvent(k); if (r2 != 0) return r2; }
    return rc;
}

// The payload-dependent part (Host header, SQL filters, HPACK, Kafka decode) runs under the packer's lock only; the packed
// events are appended to the caller's shard afterwards, outside it.
int GraphDS::IngestL7(const l7_req::L7Event& e, uint32_t kafka_msgs) {
    std::vector<sg_event> tmp;
    { std::lock_guard<std::mutex> g(pk_mu_); packer_.Pack(e, kafka_msgs, &tmp); }
    return Append(tmp.data(), tmp.size());
}

int GraphDS::IngestWire(const uint8_t* recs, size_t n, const uint32_t* kafka_msgs) {
    std::vector<sg_event> tmp;
    int rc = SG_OK;
    constexpr size_t kChunk = 256;                                // records packed per hold of the packer lock
    for (size_t i0 = 0; i0 < n; i0 += kChunk) {
        tmp.clear();
        {
            std::lock_guard<std::mutex> g(pk_mu_);
            for (size_t i = i0; i < n && i < i0 + kChunk; i++) packer_.PackWire(recs + i * l7_req::kWireSize, kafka_msgs ? kafka_msgs[i] : 1u, &tmp);
        }
        const int r2 = Append(tmp.data(), tmp.size());
        if (r2 != SG_OK) rc = r2;
    }
    return rc;
}

int GraphDS::SetSelection(uint32_t k, float min_score) {
    if (k > SG_SELECT_MAX_K || !api_.flush_window_top) return SG_EINVAL;
    std::lock_guard<std::mutex> g(flush_mu_);
    select_ = true; sel_k_ = k; sel_min_ = min_score;
    return SG_OK;
}

long GraphDS::FlushWindow(int64_t window_end_ms) {
    std::lock_guard<std::mutex> fg(flush_mu_);
    std::vector<sg_edge_out> own;                  // only without sg_flush_window_view: a pageable copy of up to max_edges rows
    const sg_edge_out* rows = nullptr;
    std::vector<uint32_t> obips;
    size_t n = 0;
    std::vector<std::string> labels;
    std::vector<uint32_t> retire_now;
    // no GraphDS lock is held across the engine's window pipeline (sg_flush_window synchronises with the device): the
    // Persist* / Ingest* callers keep appending to their shards, which go to the NEXT window
    for (Shard& s : shards_) { std::lock_guard<std::mutex> g(s.mu); const int rc = FlushShard(s); if (rc != SG_OK) return rc; }
    { std::lock_guard<std::mutex> g(pk_mu_); labels = packer_.Labels(); }
    { std::lock_guard<std::mutex> g(id_mu_); retire_now.swap(retired_); }     // ids whose last IP went away before this window closed
    api_.set_label_count(h_, (uint32_t)labels.size());
    int rc;
    size_t n_conv = 0;                             // rows handed to the sink: all of them, or the selected ones
    if (select_) {                                 // only the selected rows leave the device
        own.resize(sel_k_ ? std::min<size_t>(sel_k_, max_edges_) : max_edges_);
        size_t n_sel = 0;
        rc = api_.flush_window_top(h_, (uint64_t)window_end_ms, sel_k_, sel_min_, own.data(), nullptr, own.size(), &n_sel, &n);
        rows = own.data(); n_conv = std::min(n_sel, own.size());
    }
    else if (api_.flush_window_view) { rc = api_.flush_window_view(h_, (uint64_t)window_end_ms, &rows, &n); n_conv = n; }     // rows stay valid: flush_mu_ is held
    else { own.resize(max_edges_); rc = api_.flush_window(h_, (uint64_t)window_end_ms, own.data(), own.size(), &n); rows = own.data(); n = std::min(n, own.size()); n_conv = n; }
    if (rc != SG_OK) return rc;
    // the label table again, AFTER the window has closed: a feeder may have interned a label and pushed its event into this
    // window between the first snapshot and the close (labels are append-only, so the later snapshot is a superset)
    { std::lock_guard<std::mutex> g(pk_mu_); if (packer_.Labels().size() != labels.size()) labels = packer_.Labels(); }
    {
        size_t no = 0;
        api_.window_outbound_ips(h_, nullptr, 0, &no);
        obips.resize(no);
        if (no) api_.window_outbound_ips(h_, obips.data(), no, &no);
    }
    last_labels_ = labels; last_obips_ = obips;        // for WorkloadEdges
    std::vector<EdgeRow> out(n_conv);
    auto name = [&](uint32_t ref, std::string* type, std::string* uid) {
        const uint32_t t = SG_REF_TYPE(ref), v = SG_REF_VALUE(ref);
        if (t == SG_REF_KNOWN && v < uid_of_.size()) { *type = kind_of_[v] == SG_NODE_SERVICE ? "service" : "pod"; *uid = uid_of_[v]; }
        else if (t == SG_REF_LABEL && v < labels.size()) { *type = "outbound"; *uid = labels[v]; }
        else if (t == SG_REF_OBIP && v < obips.size()) { *type = "outbound"; *uid = FormatIPv4(obips[v]); }
        else { *type = "unknown"; uid->clear(); }
    };
    {
        std::lock_guard<std::mutex> g(id_mu_);       // uid_of_ / kind_of_ are appended to by PersistPod / PersistService
        for (size_t i = 0; i < n_conv; i++) {
            const sg_edge_out& r = rows[i]; EdgeRow& o = out[i];
            name(r.from_ref, &o.FromType, &o.FromUID); name(r.to_ref, &o.ToType, &o.ToUID);
            o.Count = r.count; o.ErrCount = r.err_count; o.SumNs = r.sum_ns; o.MaxNs = r.max_ns; o.SumSqUs = r.sumsq_us;
            o.Score = r.score; o.LatZ = r.lat_z; o.ErrRatio = r.err_ratio; o.Alive = r.alive; o.P50Us = r.p50_us; o.P99Us = r.p99_us;
        }
    }
    {   // the window that could still name the retired ids has been read: they may be handed out again, unless an IP
        // was bound to them in the meantime
        std::lock_guard<std::mutex> g(id_mu_);
        for (uint32_t id : retire_now) {
            if (refs_[id] != 0 || uid_of_[id].empty()) continue;
            auto it = ids_.find(uid_of_[id]);
            if (it != ids_.end() && it->second == id) ids_.erase(it);
            if (kind_of_[id] == SG_NODE_POD) { pod_owner_.erase(uid_of_[id]); if (groups_on_) AssignGroup(id, kNoId); }
            else if (groups_on_ && id < node_group_.size()) AssignGroup(id, kNoId);   // (a Service that was bound; never assigned: no call)
            uid_of_[id].clear(); kind_of_[id] = 0; free_ids_.push_back(id); live_ids_--;
        }
    }
    if (sink_) { const int rc2 = sink_->PersistEdges(window_end_ms, out); if (rc2 != 0) return rc2; }
    return (long)n;
}

}  // namespace alaz
