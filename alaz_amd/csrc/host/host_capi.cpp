// host_capi.cpp — flat C entry points over the C++ host side, for the Python test harness and
// for embedding.  `sgh_graphds_create(NULL, ...)` wires GraphDS to a recording stand-in of the
// engine API (host-logic tests, no GPU); a library path wires it to the real libservicegraph.so.
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "graph_ds.hpp"
#include "edges_payload.hpp"
#include "sockline.hpp"

using namespace alaz;

namespace {

// ---- recording stand-in for the engine (host-logic tests only; computes nothing) ----
struct MockEngine {
    std::vector<sg_event> events;
    std::vector<std::array<uint32_t, 3>> table_ops;   // {op: 1 upsert_pod 2 delete_pod 3 upsert_svc 4 delete_svc, ip, id}
    uint32_t label_count = 0; uint32_t flushes = 0; uint32_t max_known = 0x3FFFFFFFu;
    uint32_t top_flushes = 0, top_k = 0; float top_min = 0;             // flush_window_top: calls, the last k and min_score
    std::vector<std::array<uint32_t, 2>> group_ops;   // {node id, group} of every sg_group_assign pair; {0xFFFFFFFE, max_groups} of every sg_set_groups
    std::vector<std::array<uint64_t, 4>> k15_ops;      // {1, shift, warmup, ttl} per sg_set_group_trend, {2, silent_windows, min_seen, max_rows} per sg_set_group_vanished (NULL: ~0 in the three), {3, by, k, the bits of min_value} per sg_window_groups_top
    std::vector<std::array<uint64_t, 4>> k16_ops;      // {1, on, 0, 0} per sg_set_group_nodes, {2, shift, warmup, ttl} per sg_set_group_node_trend (NULL: ~0 in the three), {3, by, k, the bits of min_value} per sg_window_group_nodes_top
    std::vector<std::array<uint64_t, 4>> k17_ops;      // {1, iters, damping_q8, seed} per sg_set_group_rank (NULL: ~0 in the three), {2, k, the bits of min_share, cap} per sg_window_group_rank_top
    std::vector<std::array<uint64_t, 4>> k21_ops;      // {1, spaces, permille, shift (NULL: ~0)} per sg_set_quantile_trend, {2 / 3 / 4, cap, 0, 0} per sg_window_node_quantile_trend / sg_window_group_quantile_trend / sg_window_group_node_quantile_trend, {5, by, k, the bits of min_value} per sg_window_group_nodes_top_tail
    std::vector<std::array<uint64_t, 4>> k23_ops;      // {1, spaces, shift (NULL: ~0), rate_floor | load_floor_ns << 32} per sg_set_traffic_trend, {2, by, k, the bits of min_value} per sg_window_group_nodes_top_traffic
    std::vector<std::array<uint64_t, 4>> k25_ops;      // {1, min_replicas | tail_permille << 32 (NULL: ~0), min_requests, min_err_excess_q20 | min_lat_ratio_q10 << 32} per sg_set_replicas, {2, n_index, cap, 0} per sg_window_replicas, {3, by, k, min_value} per sg_window_replicas_top
    std::vector<std::array<uint64_t, 4>> k24_ops;      // {1, spaces, latency_bin | long_windows << 32 (NULL: ~0), min_requests} per sg_set_slo, {2, space, ref, objective} per ref of sg_slo_assign, {3, cap, 0, 0} per sg_window_group_node_slo, {4, by, k, min_value_q10} per sg_window_group_nodes_top_slo
    std::vector<std::array<uint64_t, 4>> k20_ops;      // {1, spaces, n_q, the first four per-mille 16 bits each} per sg_set_quantiles, {2 / 3 / 4, n_index (~0: no index), cap, 0} per sg_window_node_quantiles / sg_window_group_quantiles / sg_window_group_node_quantiles
    size_t k20_nq = 2;
    std::vector<std::array<uint64_t, 4>> k19_ops;      // {1, quiet_windows, max_tracks, reserved} per sg_set_group_tracks (NULL: ~0 in the three), {2, cap, 0, 0} per sg_window_group_incident_tracks, {3, cap, 0, 0} per sg_window_group_tracks_ended
    std::vector<std::array<uint64_t, 4>> k18_ops;      // {1, by, the bits of min_value, reserved} per sg_set_group_incidents (NULL: ~0 in the three), {2, cap, 0, 0} per sg_window_group_incidents, {3, n_index, cap, 0} per sg_window_group_node_incident
    std::vector<std::array<uint64_t, 4>> k22_ops;      // {1, max_incidents, max_hops, 0} per sg_set_group_impact, {2, cap, 0, 0} per sg_window_group_impact
    std::mutex mu;                                     // like the real engine, the stand-in serialises the calls on one handle
};
#define M_LOCK(h) std::lock_guard<std::mutex> _g(reinterpret_cast<MockEngine*>(h)->mu)
int m_create(const sg_config* cfg, sg_handle* out) { auto* m = new MockEngine(); if (cfg && cfg->max_known_nodes) m->max_known = cfg->max_known_nodes; *out = reinterpret_cast<sg_handle>(m); return SG_OK; }
int m_destroy(sg_handle h) { delete reinterpret_cast<MockEngine*>(h); return SG_OK; }
int m_upsert_pod(sg_handle h, uint32_t ip, uint32_t id) { M_LOCK(h); auto* m = reinterpret_cast<MockEngine*>(h); if (id >= m->max_known) return SG_ENOSPC; m->table_ops.push_back({1u, ip, id}); return SG_OK; }
int m_delete_pod(sg_handle h, uint32_t ip) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->table_ops.push_back({2u, ip, 0u}); return SG_OK; }
int m_upsert_svc(sg_handle h, uint32_t ip, uint32_t id) { M_LOCK(h); auto* m = reinterpret_cast<MockEngine*>(h); if (id >= m->max_known) return SG_ENOSPC; m->table_ops.push_back({3u, ip, id}); return SG_OK; }
int m_delete_svc(sg_handle h, uint32_t ip) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->table_ops.push_back({4u, ip, 0u}); return SG_OK; }
int m_labels(sg_handle h, uint32_t n) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->label_count = n; return SG_OK; }
int m_ingest(sg_handle h, const sg_event* ev, size_t n) { M_LOCK(h); auto* m = reinterpret_cast<MockEngine*>(h); m->events.insert(m->events.end(), ev, ev + n); return SG_OK; }
int m_flush(sg_handle h, uint64_t, sg_edge_out*, size_t, size_t* n) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->flushes++; if (n) *n = 0; return SG_OK; }
int m_flush_top(sg_handle h, uint64_t, uint32_t k, float min_score, sg_edge_out*, uint32_t*, size_t, size_t* n_sel, size_t* n) {
    M_LOCK(h); auto* m = reinterpret_cast<MockEngine*>(h); m->top_flushes++; m->top_k = k; m->top_min = min_score;
    if (n_sel) *n_sel = 0;
    if (n) *n = 0;
    return SG_OK;
}
int m_set_groups(sg_handle h, const sg_group_params* p) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->group_ops.push_back({0xFFFFFFFEu, p ? p->max_groups : 0xFFFFFFFFu}); return SG_OK; }
int m_group_assign(sg_handle h, const uint32_t* ids, const uint32_t* gs, size_t n) {
    M_LOCK(h); auto* m = reinterpret_cast<MockEngine*>(h);
    for (size_t i = 0; i < n; i++) m->group_ops.push_back({ids[i], gs[i]});
    return SG_OK;
}
int m_window_groups(sg_handle, sg_group_edge*, size_t, size_t* n) { if (n) *n = 0; return SG_OK; }
// K15's stand-ins answer with fixed rows, so that what GraphDS makes of them can be checked: four group edges' trend rows
// (windows_seen = 1 + the group edge's index); two vanished entries — workload 1 -> workload 0 with row 2, and ungrouped KNOWN 7 ->
// outbound 10.0.0.1 — of three counted; a selection of group edges 3 and 0 of four (workload 1 -> workload 0, workload 0 -> KNOWN 0)
int m_set_group_trend(sg_handle h, const sg_trend_params* p) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k15_ops.push_back({1u, p ? p->shift : ~0ull, p ? p->warmup : ~0ull, p ? p->ttl : ~0ull}); return SG_OK;
}
int m_set_group_vanished(sg_handle h, const sg_vanished_params* p) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k15_ops.push_back({2u, p ? p->silent_windows : ~0ull, p ? p->min_seen : ~0ull, p ? p->max_rows : ~0ull}); return SG_OK;
}
int m_window_group_trend(sg_handle, const uint32_t* idx, size_t n_idx, sg_edge_trend* out, size_t cap, size_t* n) {
    const size_t N = idx ? n_idx : 4;
    if (n) *n = N;
    for (size_t i = 0; out && i < std::min(N, cap); i++) out[i] = sg_edge_trend{0.5f, -0.25f, 2.0f, 1u + (idx ? idx[i] : (uint32_t)i)};
    return SG_OK;
}
int m_window_group_vanished(sg_handle, sg_edge_vanished* out, size_t cap, size_t* n) {
    if (n) *n = 3;                                                // (one more than max_rows = 2 holds)
    const sg_edge_vanished v[2] = {{1ull, 0ull, 1000.0, 10.0, 0.0, 0.0, 5u, 7u, 2u, 0u},
                                   {(1ull << 32) | 7ull, (3ull << 32) | 0x0A000001ull, 2000.0, 20.0, 1.0, 2.0, 6u, 7u, 0xFFFFFFFFu, 0u}};
    for (size_t i = 0; out && i < std::min<size_t>(2, cap); i++) out[i] = v[i];
    return SG_OK;
}
int m_window_groups_top(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_group_edge* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    uint32_t bits; std::memcpy(&bits, &min_value, 4);
    reinterpret_cast<MockEngine*>(h)->k15_ops.push_back({3u, by, k, bits});
    if (n_sel) *n_sel = 2;
    if (n) *n = 4;
    sg_group_edge e[2] = {};
    e[0].from_ref = SG_MAKE_REF(SG_REF_GROUP, 1); e[0].to_ref = SG_MAKE_REF(SG_REF_GROUP, 0); e[0].count = 9; e[0].score_max = 0.75f;
    e[1].from_ref = SG_MAKE_REF(SG_REF_GROUP, 0); e[1].to_ref = SG_MAKE_REF(SG_REF_KNOWN, 0); e[1].count = 4; e[1].score_max = 0.5f;
    const uint32_t at[2] = {3u, 0u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K16's stand-ins answer with fixed rows: three workload rows — workload 1, workload 0 (note: the order of the group key is the
// engine's, the stand-in's is arbitrary) and ungrouped KNOWN 0 — their trend rows (in_seen = 1 + the row's index), and a selection
// of rows 2 and 0 of three
static sg_node_out m_node(uint32_t ref, uint64_t out_count, uint64_t in_count, uint32_t out_edges, uint32_t in_edges, float score) {
    sg_node_out o{}; o.ref = ref; o.out_count = out_count; o.in_count = in_count; o.out_edges = out_edges; o.in_edges = in_edges; o.score = score;
    o.out_worst_row = o.in_worst_row = 0xFFFFFFFFu;
    return o;
}
int m_set_group_nodes(sg_handle h, int on) { M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k16_ops.push_back({1u, (uint64_t)on, 0u, 0u}); return SG_OK; }
int m_set_group_node_trend(sg_handle h, const sg_trend_params* p) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k16_ops.push_back({2u, p ? p->shift : ~0ull, p ? p->warmup : ~0ull, p ? p->ttl : ~0ull}); return SG_OK;
}
int m_window_group_nodes(sg_handle, sg_node_out* out, size_t cap, size_t* n) {
    const sg_node_out v[3] = {m_node(SG_MAKE_REF(SG_REF_GROUP, 1), 9, 0, 2, 0, 0.75f), m_node(SG_MAKE_REF(SG_REF_GROUP, 0), 4, 9, 1, 1, 0.5f),
                              m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    if (n) *n = 3;
    for (size_t i = 0; out && i < std::min<size_t>(3, cap); i++) out[i] = v[i];
    return SG_OK;
}
int m_window_group_node_trend(sg_handle, const uint32_t* idx, size_t n_idx, sg_node_trend* out, size_t cap, size_t* n) {
    const size_t N = idx ? n_idx : 3;
    if (n) *n = N;
    for (size_t i = 0; out && i < std::min(N, cap); i++) {
        sg_node_trend t{}; t.in_lat_dev = 0.5f; t.out_lat_dev = -0.25f; t.in_seen = 1u + (idx ? idx[i] : (uint32_t)i); t.out_seen = 7u;
        out[i] = t;
    }
    return SG_OK;
}
int m_window_group_nodes_top(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    uint32_t bits; std::memcpy(&bits, &min_value, 4);
    reinterpret_cast<MockEngine*>(h)->k16_ops.push_back({3u, by, k, bits});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f), m_node(SG_MAKE_REF(SG_REF_GROUP, 1), 9, 0, 2, 0, 0.75f)};
    const uint32_t at[2] = {2u, 0u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K17's stand-ins: the switch recorded, and a selection of rows 1 and 2 of three (workload 0 with three quarters of the mass, then
// ungrouped KNOWN 0)
int m_set_group_rank(sg_handle h, const sg_rank_params* p) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k17_ops.push_back({1u, p ? p->iters : ~0ull, p ? p->damping_q8 : ~0ull, p ? p->seed : ~0ull}); return SG_OK;
}
int m_window_group_rank_top(sg_handle h, uint32_t k, float min_share, sg_node_out* out, sg_node_rank* rank_out, uint32_t* idx, size_t cap, size_t* n_sel,
                            size_t* n) {
    M_LOCK(h);
    uint32_t bits; std::memcpy(&bits, &min_share, 4);
    reinterpret_cast<MockEngine*>(h)->k17_ops.push_back({2u, k, bits, (uint64_t)cap});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_GROUP, 0), 4, 9, 1, 1, 0.5f), m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    const sg_node_rank r[2] = {{3ull << 54, SG_MAKE_REF(SG_REF_GROUP, 0), 0.75f}, {1ull << 53, SG_MAKE_REF(SG_REF_KNOWN, 0), 0.125f}};
    const uint32_t at[2] = {1u, 2u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (rank_out) rank_out[i] = r[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K18's stand-ins: the switch recorded; two incidents over three workload rows (rows 0 and 2 in incident 0 with culprit 2, row 1
// alone in incident 1 without a culprit)
int m_set_group_incidents(sg_handle h, const sg_incident_params* p) {
    M_LOCK(h);
    uint32_t bits = 0; if (p) std::memcpy(&bits, &p->min_value, 4);
    reinterpret_cast<MockEngine*>(h)->k18_ops.push_back({1u, p ? p->by : ~0ull, p ? bits : ~0ull, p ? p->reserved : ~0ull}); return SG_OK;
}
int m_window_group_incidents(sg_handle h, sg_incident_out* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k18_ops.push_back({2u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 2;
    sg_incident_out e[2] = {};
    e[0].count = 9; e[0].err = 2; e[0].sum_ns = 900; e[0].score_q32 = 3ull << 31; e[0].rank_sum = 3ull << 54; e[0].first_node = 0; e[0].nodes = 2;
    e[0].edges = 2; e[0].worst_row = 1; e[0].top_node = 2; e[0].culprit_node = 2; e[0].value_max = 0.75f;
    e[1].count = 4; e[1].first_node = 1; e[1].nodes = 1; e[1].edges = 1; e[1].worst_row = 2; e[1].top_node = 1; e[1].culprit_node = SG_NO_INCIDENT;
    e[1].value_max = 0.5f;
    for (size_t i = 0; out && i < std::min<size_t>(2, cap); i++) out[i] = e[i];
    return SG_OK;
}
// K22's stand-ins: the switch recorded; the impact rows of K18's two incidents (incident 0: one exposed row, row 1, one hop away,
// which is an entry; incident 1: nothing exposed)
int m_set_group_impact(sg_handle h, uint32_t max_incidents, uint32_t max_hops) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k22_ops.push_back({1u, max_incidents, max_hops, 0u}); return SG_OK;
}
int m_window_group_impact(sg_handle h, uint64_t* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k22_ops.push_back({2u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 2;
    const uint64_t e[2][SG_IMPACT_WORDS] = {{1, 1, 1ull << 32 | 1, 1, 40, 3, 7, 2}, {0, 0, 0xFFFFFFFFull, 1, 4, 0, 0, 0}};
    for (size_t i = 0; out && i < std::min<size_t>(2, cap); i++) std::memcpy(out + i * SG_IMPACT_WORDS, e[i], sizeof e[i]);
    return SG_OK;
}
// K19's stand-ins: the switch recorded; the tracks of K18's two incidents (track 4 continued into its third window, track 7 opened
// as a split of it) and one ended entry
int m_set_group_tracks(sg_handle h, const sg_track_params* p) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k19_ops.push_back({1u, p ? p->quiet_windows : ~0ull, p ? p->max_tracks : ~0ull, p ? p->reserved : ~0ull}); return SG_OK;
}
int m_window_group_incident_tracks(sg_handle h, sg_incident_track* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k19_ops.push_back({2u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 2;
    const sg_incident_track e[2] = {{4u, SG_NO_TRACK, 1u, 3u, 2u, 0u, 0u, 0u}, {7u, 4u, 3u, 1u, 0u, 0u, 1u, SG_TRACK_NEW | SG_TRACK_SPLIT}};
    for (size_t i = 0; out && i < std::min<size_t>(2, cap); i++) out[i] = e[i];
    return SG_OK;
}
int m_window_group_tracks_ended(sg_handle h, sg_track_entry* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k19_ops.push_back({3u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 1;
    const sg_track_entry e = {5u, 4u, 1u, 2u, 2u, 3u, 17ull, 2ull};
    if (out && cap) out[0] = e;
    return SG_OK;
}
// K20's stand-ins: the switch recorded; three entities without an index, word k of the rows = 10 * which + k
int m_set_quantiles(sg_handle h, uint32_t spaces, const uint32_t* permille, size_t n_q) {
    M_LOCK(h);
    auto* m = reinterpret_cast<MockEngine*>(h);
    uint64_t packed = 0;
    for (size_t k = 0; k < std::min<size_t>(n_q, 4); k++) packed |= (uint64_t)(permille[k] & 0xFFFFu) << (16 * k);
    m->k20_ops.push_back({1u, spaces, (uint64_t)n_q, packed});
    if (n_q > SG_Q_MAX) return SG_EINVAL;
    m->k20_nq = n_q ? n_q : 2;
    return SG_OK;
}
int m_quantile_rows(sg_handle h, uint64_t which, size_t sides, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) {
    M_LOCK(h);
    auto* m = reinterpret_cast<MockEngine*>(h);
    m->k20_ops.push_back({which, idx ? (uint64_t)n_idx : ~0ull, (uint64_t)cap, 0u});
    const size_t rows = idx ? n_idx : 3;
    if (n) *n = rows;
    for (size_t k = 0; out && k < std::min(rows, cap) * sides * m->k20_nq; k++) out[k] = (uint32_t)(10 * which + k);
    return SG_OK;
}
int m_window_node_quantiles(sg_handle h, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) { return m_quantile_rows(h, 2, 2, idx, n_idx, out, cap, n); }
int m_window_group_quantiles(sg_handle h, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) { return m_quantile_rows(h, 3, 1, idx, n_idx, out, cap, n); }
int m_window_group_node_quantiles(sg_handle h, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) { return m_quantile_rows(h, 4, 2, idx, n_idx, out, cap, n); }
// K21's stand-ins: the switch recorded; three rows a space (in_seen / windows_seen = 10 * which + the row's index, lat_dev 8 + which);
// the tail selection is K16's with rows 1 and 2 of three
int m_set_quantile_trend(sg_handle h, uint32_t spaces, uint32_t permille, const sg_trend_params* p) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k21_ops.push_back({1u, spaces, permille, p ? p->shift : ~0ull}); return spaces > 7u ? SG_EINVAL : SG_OK;
}
static int m_tail_node_rows(sg_handle h, uint64_t which, sg_node_trend* out, size_t cap, size_t* n) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k21_ops.push_back({which, (uint64_t)cap, 0u, 0u});
    if (n) *n = 3;
    for (size_t i = 0; out && i < std::min<size_t>(3, cap); i++) { sg_node_trend t{}; t.in_lat_dev = 8.f + (float)which; t.in_seen = (uint32_t)(10 * which + i); out[i] = t; }
    return SG_OK;
}
int m_window_node_quantile_trend(sg_handle h, const uint32_t*, size_t, sg_node_trend* out, size_t cap, size_t* n) { return m_tail_node_rows(h, 2, out, cap, n); }
int m_window_group_node_quantile_trend(sg_handle h, const uint32_t*, size_t, sg_node_trend* out, size_t cap, size_t* n) { return m_tail_node_rows(h, 4, out, cap, n); }
int m_window_group_quantile_trend(sg_handle h, const uint32_t*, size_t, sg_edge_trend* out, size_t cap, size_t* n) {
    M_LOCK(h); reinterpret_cast<MockEngine*>(h)->k21_ops.push_back({3u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 3;
    for (size_t i = 0; out && i < std::min<size_t>(3, cap); i++) { sg_edge_trend t{}; t.lat_dev = 11.f; t.windows_seen = (uint32_t)(30 + i); out[i] = t; }
    return SG_OK;
}
int m_window_group_nodes_top_tail(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    uint32_t bits; std::memcpy(&bits, &min_value, 4);
    reinterpret_cast<MockEngine*>(h)->k21_ops.push_back({5u, by, k, bits});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_GROUP, 0), 4, 9, 1, 1, 0.5f), m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    const uint32_t at[2] = {1u, 2u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K23's stand-ins: the switch recorded; the traffic selection is K16's with rows 1 and 2 of three
int m_set_traffic_trend(sg_handle h, uint32_t spaces, const sg_traffic_params* p) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k23_ops.push_back({1u, spaces, p ? p->shift : ~0ull, p ? (uint64_t)p->rate_floor | p->load_floor_ns << 32 : 0u});
    return spaces > 15u ? SG_EINVAL : SG_OK;
}
int m_window_group_nodes_top_traffic(sg_handle h, uint32_t by, uint32_t k, float min_value, sg_node_out* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    uint32_t bits; std::memcpy(&bits, &min_value, 4);
    reinterpret_cast<MockEngine*>(h)->k23_ops.push_back({2u, by, k, bits});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_GROUP, 0), 4, 9, 1, 1, 0.5f), m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    const uint32_t at[2] = {1u, 2u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K24's stand-ins: the switch and the objectives recorded; three SLO rows, row j's word w = 100 j + w; the selection is K16's with
// rows 1 and 2 of three
int m_set_slo(sg_handle h, uint32_t spaces, const sg_slo_params* p) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k24_ops.push_back({1u, spaces, p ? (uint64_t)p->latency_bin | (uint64_t)p->long_windows << 32 : ~0ull, p ? p->min_requests : 0u});
    return (spaces & ~5u) ? SG_EINVAL : SG_OK;
}
int m_slo_assign(sg_handle h, uint32_t space, const uint32_t* refs, const uint32_t* obj, size_t n) {
    M_LOCK(h);
    for (size_t i = 0; i < n; i++) reinterpret_cast<MockEngine*>(h)->k24_ops.push_back({2u, space, refs[i], obj[i]});
    return SG_OK;
}
int m_window_group_node_slo(sg_handle h, const uint32_t*, size_t, uint64_t* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k24_ops.push_back({3u, (uint64_t)cap, 0u, 0u});
    if (n) *n = 3;
    for (size_t j = 0; out && j < std::min<size_t>(3, cap); j++) for (size_t w = 0; w < SG_SLO_WORDS; w++) out[j * SG_SLO_WORDS + w] = 100 * j + w;
    return SG_OK;
}
int m_window_group_nodes_top_slo(sg_handle h, uint32_t by, uint32_t k, uint32_t min_value_q10, sg_node_out* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k24_ops.push_back({4u, by, k, min_value_q10});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_GROUP, 0), 4, 9, 1, 1, 0.5f), m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    const uint32_t at[2] = {1u, 2u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
// K25's stand-ins: the switch recorded; the pod row of node row j is a member of workload row 1 (word 0), its words 1 .. 11 are
// 100 j + w; the selection gives node rows 2 and 0 of three: KNOWN 1, then KNOWN 0
int m_set_replicas(sg_handle h, const sg_replica_params* p) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k25_ops.push_back({1u, p ? (uint64_t)p->min_replicas | (uint64_t)p->tail_permille << 32 : ~0ull, p ? p->min_requests : 0u,
                                                         p ? (uint64_t)p->min_err_excess_q20 | (uint64_t)p->min_lat_ratio_q10 << 32 : 0u});
    return p && p->min_replicas == 1 ? SG_EINVAL : SG_OK;
}
int m_window_replicas(sg_handle h, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k25_ops.push_back({2u, idx ? (uint64_t)n_idx : ~0ull, (uint64_t)cap, 0u});
    const size_t N = idx ? n_idx : 3;
    if (n) *n = N;
    for (size_t i = 0; out && i < std::min(N, cap); i++) {
        const uint32_t j = idx ? idx[i] : (uint32_t)i;
        out[i * SG_REPLICA_WORDS] = 1u;
        for (uint32_t w = 1; w < SG_REPLICA_WORDS; w++) out[i * SG_REPLICA_WORDS + w] = 100 * j + w;
    }
    return SG_OK;
}
int m_window_replicas_top(sg_handle h, uint32_t by, uint32_t k, uint32_t min_value, sg_node_out* out, uint32_t* idx, size_t cap, size_t* n_sel, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k25_ops.push_back({3u, by, k, min_value});
    if (n_sel) *n_sel = 2;
    if (n) *n = 3;
    const sg_node_out e[2] = {m_node(SG_MAKE_REF(SG_REF_KNOWN, 1), 0, 7, 0, 1, 0.5f), m_node(SG_MAKE_REF(SG_REF_KNOWN, 0), 0, 4, 0, 1, 0.25f)};
    const uint32_t at[2] = {2u, 0u};
    for (size_t i = 0; i < std::min<size_t>(2, cap); i++) { if (out) out[i] = e[i]; if (idx) idx[i] = at[i]; }
    return SG_OK;
}
int m_window_group_node_incident(sg_handle h, const uint32_t* idx, size_t n_idx, uint32_t* out, size_t cap, size_t* n) {
    M_LOCK(h);
    reinterpret_cast<MockEngine*>(h)->k18_ops.push_back({3u, (uint64_t)n_idx, (uint64_t)cap, 0u});
    const uint32_t inc[3] = {0u, 1u, 0u};
    const size_t m = idx ? n_idx : 3;
    if (n) *n = m;
    for (size_t i = 0; out && i < std::min(m, cap); i++) { const uint32_t v = idx ? idx[i] : (uint32_t)i; if (v >= 3) return SG_EINVAL; out[i] = inc[v]; }
    return SG_OK;
}
int m_obips(sg_handle, uint32_t*, size_t, size_t* n) { if (n) *n = 0; return SG_OK; }
const char* m_err(sg_handle) { return ""; }

struct CollectSink : EdgeSink {
    std::vector<EdgeRow> rows; int64_t window_end = 0;
    int PersistEdges(int64_t w, const std::vector<EdgeRow>& r) override { window_end = w; rows = r; return 0; }
};

// the inner data store of the tests: the out-of-scope BackendDS stand-in, counting what reaches it
struct CountingDataStore : datastore::NullDataStore {
    std::atomic<uint64_t> requests{0}, kafka{0}, alive{0}, pods{0}, services{0};
    int PersistPod(const datastore::Pod&, const std::string&) override { pods++; return 0; }
    int PersistService(const datastore::Service&, const std::string&) override { services++; return 0; }
    int PersistRequest(const datastore::Request*) override { requests++; return 0; }
    int PersistKafkaEvent(const datastore::KafkaEvent*) override { kafka++; return 0; }
    int PersistAliveConnection(const datastore::AliveConnection*) override { alive++; return 0; }
};

struct HostCtx {
    void* dl = nullptr; SgApi api; sg_handle h = nullptr; bool mock = false;
    CountingDataStore inner; CollectSink sink;
    std::unique_ptr<GraphDS> ds;
    ConnTracker conns;                 // f-2: TCP connect events -> socket lines -> alive connections
};

}  // namespace

extern "C" {

struct sgh_edge_row {
    char from_type[12], to_type[12], from_uid[160], to_uid[160];
    uint32_t count, err_count; uint64_t sum_ns, max_ns, sumsq_us; float score, lat_z, err_ratio; uint32_t alive; uint32_t p50_us, p99_us;
};

void* sgh_packer_create(void) { return new L7Packer(); }
void sgh_packer_destroy(void* p) { delete static_cast<L7Packer*>(p); }
void sgh_packer_known_ip(void* p, uint32_t ip, int add) { static_cast<L7Packer*>(p)->SetPodIP(ip, add != 0); }
size_t sgh_packer_pack_wire(void* p, const uint8_t* recs, size_t n, const uint32_t* kafka_msgs, sg_event* out, size_t cap) {
    auto* pk = static_cast<L7Packer*>(p);
    std::vector<sg_event> v; v.reserve(n);
    for (size_t i = 0; i < n; i++) pk->PackWire(recs + i * l7_req::kWireSize, kafka_msgs ? kafka_msgs[i] : 1u, &v);
    const size_t m = std::min(cap, v.size());
    if (m) std::memcpy(out, v.data(), m * sizeof(sg_event));
    return v.size();
}
// the same through the user-space L7Event (DecodeWire with the full 1 KiB copy, then L7Packer::Pack): what a caller holding
// l7_req.L7Event objects gets; must equal sgh_packer_pack_wire record for record (tests)
size_t sgh_packer_pack_wire_full(void* p, const uint8_t* recs, size_t n, const uint32_t* kafka_msgs, sg_event* out, size_t cap) {
    auto* pk = static_cast<L7Packer*>(p);
    std::vector<sg_event> v; v.reserve(n);
    auto e = std::make_unique<l7_req::L7Event>();
    for (size_t i = 0; i < n; i++) { l7_req::DecodeWire(recs + i * l7_req::kWireSize, e.get(), true); pk->Pack(*e, kafka_msgs ? kafka_msgs[i] : 1u, &v); }
    const size_t m = std::min(cap, v.size());
    if (m) std::memcpy(out, v.data(), m * sizeof(sg_event));
    return v.size();
}
static size_t join_labels(const std::vector<std::string>& l, char* buf, size_t cap) {
    std::string s;
    for (size_t i = 0; i < l.size(); i++) { if (i) s.push_back('\n'); s += l[i]; }
    if (buf && cap) { const size_t m = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), m); buf[m] = 0; }
    return l.size();
}
size_t sgh_packer_labels(void* p, char* buf, size_t cap) { return join_labels(static_cast<L7Packer*>(p)->Labels(), buf, cap); }
uint64_t sgh_packer_dropped_parse(void* p) { return static_cast<L7Packer*>(p)->DroppedParse(); }
void sgh_parse_http(const char* req, size_t len, char* m, char* p, char* v, char* h, size_t cap) {
    std::string sm, sp, sv, sh;
    ParseHttpPayload(req, len, &sm, &sp, &sv, &sh);
    auto put = [&](char* d, const std::string& s) { const size_t k = std::min(cap - 1, s.size()); std::memcpy(d, s.data(), k); d[k] = 0; };
    put(m, sm); put(p, sp); put(v, sv); put(h, sh);
}

void* sgh_graphds_create2(const char* engine_lib, const sg_config* cfg, size_t batch, int divert_requests);
void* sgh_graphds_create(const char* engine_lib, const sg_config* cfg, size_t batch) { return sgh_graphds_create2(engine_lib, cfg, batch, 0); }
void* sgh_graphds_create2(const char* engine_lib, const sg_config* cfg, size_t batch, int divert_requests) {
    auto c = std::make_unique<HostCtx>();
    if (engine_lib) {
        c->dl = dlopen(engine_lib, RTLD_NOW | RTLD_GLOBAL);
        if (!c->dl || !SgApi::FromLibrary(c->dl, &c->api)) return nullptr;
    } else {
        c->mock = true;
        c->api.create = m_create; c->api.destroy = m_destroy; c->api.upsert_pod = m_upsert_pod; c->api.delete_pod = m_delete_pod;
        c->api.upsert_service = m_upsert_svc; c->api.delete_service = m_delete_svc; c->api.set_label_count = m_labels; c->api.ingest = m_ingest;
        c->api.flush_window = m_flush; c->api.window_outbound_ips = m_obips; c->api.last_error = m_err; c->api.flush_window_top = m_flush_top;
        c->api.set_groups = m_set_groups; c->api.group_assign = m_group_assign; c->api.window_groups = m_window_groups;
        c->api.set_group_trend = m_set_group_trend; c->api.window_group_trend = m_window_group_trend; c->api.set_group_vanished = m_set_group_vanished;
        c->api.window_group_vanished = m_window_group_vanished; c->api.window_groups_top = m_window_groups_top;
        c->api.set_group_nodes = m_set_group_nodes; c->api.window_group_nodes = m_window_group_nodes; c->api.set_group_node_trend = m_set_group_node_trend;
        c->api.window_group_node_trend = m_window_group_node_trend; c->api.window_group_nodes_top = m_window_group_nodes_top;
        c->api.set_group_rank = m_set_group_rank; c->api.window_group_rank_top = m_window_group_rank_top;
        c->api.set_group_tracks = m_set_group_tracks; c->api.window_group_incident_tracks = m_window_group_incident_tracks;
        c->api.window_group_tracks_ended = m_window_group_tracks_ended;
        c->api.set_quantiles = m_set_quantiles; c->api.window_node_quantiles = m_window_node_quantiles;
        c->api.window_group_quantiles = m_window_group_quantiles; c->api.window_group_node_quantiles = m_window_group_node_quantiles;
        c->api.set_quantile_trend = m_set_quantile_trend; c->api.window_node_quantile_trend = m_window_node_quantile_trend;
        c->api.window_group_quantile_trend = m_window_group_quantile_trend; c->api.window_group_node_quantile_trend = m_window_group_node_quantile_trend;
        c->api.window_group_nodes_top_tail = m_window_group_nodes_top_tail;
        c->api.set_traffic_trend = m_set_traffic_trend; c->api.window_group_nodes_top_traffic = m_window_group_nodes_top_traffic;
        c->api.set_replicas = m_set_replicas; c->api.window_replicas = m_window_replicas; c->api.window_replicas_top = m_window_replicas_top;
        c->api.set_slo = m_set_slo; c->api.slo_assign = m_slo_assign; c->api.window_group_node_slo = m_window_group_node_slo;
        c->api.window_group_nodes_top_slo = m_window_group_nodes_top_slo;
        c->api.set_group_incidents = m_set_group_incidents; c->api.window_group_incidents = m_window_group_incidents;
        c->api.window_group_node_incident = m_window_group_node_incident;
        c->api.set_group_impact = m_set_group_impact; c->api.window_group_impact = m_window_group_impact;
    }
    if (c->api.create(cfg, &c->h) != SG_OK) return nullptr;        // no usable GPU => no GraphDS: there is no CPU fallback
    c->ds = std::make_unique<GraphDS>(&c->inner, c->api, c->h, &c->sink, cfg ? (size_t)cfg->max_edges : 1024, batch ? batch : 4096,
                                      cfg && cfg->max_known_nodes ? cfg->max_known_nodes : 0x3FFFFFFFu, divert_requests != 0);
    return c.release();
}
void sgh_graphds_destroy(void* g) { auto* c = static_cast<HostCtx*>(g); if (!c) return; c->ds.reset(); if (c->h) c->api.destroy(c->h); delete c; }
int sgh_graphds_persist_pod(void* g, const char* et, const char* uid, const char* ip) { datastore::Pod p; p.UID = uid; p.IP = ip; return static_cast<HostCtx*>(g)->ds->PersistPod(p, et); }
int sgh_graphds_persist_service(void* g, const char* et, const char* uid, const char* ip) { datastore::Service s; s.UID = uid; if (ip && *ip) s.ClusterIPs.push_back(ip); return static_cast<HostCtx*>(g)->ds->PersistService(s, et); }
// the workload view (K14): a pod with its owner, a ReplicaSet with its owner, the switch, and the last flushed window's group edges
int sgh_graphds_persist_pod_owned(void* g, const char* et, const char* uid, const char* ip, const char* owner_id) {
    datastore::Pod p; p.UID = uid; p.IP = ip; p.OwnerID = owner_id ? owner_id : "";
    return static_cast<HostCtx*>(g)->ds->PersistPod(p, et);
}
int sgh_graphds_persist_replicaset(void* g, const char* et, const char* uid, const char* owner_id) {
    datastore::ReplicaSet rs; rs.UID = uid; rs.OwnerID = owner_id ? owner_id : "";
    return static_cast<HostCtx*>(g)->ds->PersistReplicaSet(rs, et);
}
int sgh_graphds_set_workload_groups(void* g, uint32_t max_groups) { return static_cast<HostCtx*>(g)->ds->SetWorkloadGroups(max_groups); }
// the service binding: a Service with its name and namespace, the Endpoints of (namespace, name) as n (type, id) address pairs, the switch
int sgh_graphds_persist_service_named(void* g, const char* et, const char* uid, const char* ip, const char* name, const char* ns) {
    datastore::Service s; s.UID = uid; s.Name = name ? name : ""; s.Namespace = ns ? ns : "";
    if (ip && *ip) s.ClusterIPs.push_back(ip);
    return static_cast<HostCtx*>(g)->ds->PersistService(s, et);
}
int sgh_graphds_persist_endpoints(void* g, const char* et, const char* name, const char* ns, const char* const* types, const char* const* ids, size_t n) {
    datastore::Endpoints e; e.Name = name ? name : ""; e.Namespace = ns ? ns : "";
    datastore::Address a;
    for (size_t i = 0; i < n; i++) { datastore::AddressIP ip; ip.Type = types[i] ? types[i] : ""; ip.ID = ids[i] ? ids[i] : ""; a.IPs.push_back(ip); }
    if (n) e.Addresses.push_back(a);
    return static_cast<HostCtx*>(g)->ds->PersistEndpoints(e, et);
}
int sgh_graphds_set_service_binding(void* g, int on) { return static_cast<HostCtx*>(g)->ds->SetServiceBinding(on != 0); }
struct sgh_workload_edge {
    char from_type[12], to_type[12], from_uid[160], to_uid[160];
    uint64_t count, err_count, sum_ns, sumsq_us, max_ns, score_q32; uint32_t edges, from_nodes, alive, worst_row; float score_max; uint32_t pad;
};
long sgh_graphds_workload_edges(void* g, sgh_workload_edge* out, size_t cap) {
    std::vector<WorkloadEdge> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadEdges(&v);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) {
        const WorkloadEdge& r = v[i]; sgh_workload_edge& o = out[i];
        std::memset(&o, 0, sizeof o);
        std::strncpy(o.from_type, r.FromType.c_str(), sizeof o.from_type - 1); std::strncpy(o.to_type, r.ToType.c_str(), sizeof o.to_type - 1);
        std::strncpy(o.from_uid, r.FromUID.c_str(), sizeof o.from_uid - 1); std::strncpy(o.to_uid, r.ToUID.c_str(), sizeof o.to_uid - 1);
        o.count = r.Count; o.err_count = r.ErrCount; o.sum_ns = r.SumNs; o.sumsq_us = r.SumSqUs; o.max_ns = r.MaxNs; o.score_q32 = r.ScoreQ32;
        o.edges = r.Edges; o.from_nodes = r.FromNodes; o.alive = r.Alive; o.worst_row = r.WorstRow; o.score_max = r.ScoreMax;
    }
    return n;
}
// the workload baselines (K15): the two switches (a parameter 0 = its default), the last flushed window's group trend rows (as
// sg_edge_trend), a selection over its group edges and its vanished workload dependencies
int sgh_graphds_set_workload_trend(void* g, uint32_t shift, uint32_t warmup, uint32_t ttl, uint64_t max_entries) {
    sg_trend_params p{}; p.struct_size = sizeof p; p.shift = shift; p.warmup = warmup; p.ttl = ttl; p.max_entries = max_entries;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadTrend(p);
}
int sgh_graphds_set_workload_vanished(void* g, uint32_t silent_windows, uint32_t min_seen, uint32_t max_rows) {
    sg_vanished_params p{}; p.struct_size = sizeof p; p.silent_windows = silent_windows; p.min_seen = min_seen; p.max_rows = max_rows;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadVanished(p);
}
long sgh_graphds_workload_trends(void* g, sg_edge_trend* out, size_t cap) {
    std::vector<sg_edge_trend> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadTrends(&v);
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_edge_trend));
    return n;
}
static void put_workload_edge(const WorkloadEdge& r, sgh_workload_edge* o) {
    std::memset(o, 0, sizeof *o);
    std::strncpy(o->from_type, r.FromType.c_str(), sizeof o->from_type - 1); std::strncpy(o->to_type, r.ToType.c_str(), sizeof o->to_type - 1);
    std::strncpy(o->from_uid, r.FromUID.c_str(), sizeof o->from_uid - 1); std::strncpy(o->to_uid, r.ToUID.c_str(), sizeof o->to_uid - 1);
    o->count = r.Count; o->err_count = r.ErrCount; o->sum_ns = r.SumNs; o->sumsq_us = r.SumSqUs; o->max_ns = r.MaxNs; o->score_q32 = r.ScoreQ32;
    o->edges = r.Edges; o->from_nodes = r.FromNodes; o->alive = r.Alive; o->worst_row = r.WorstRow; o->score_max = r.ScoreMax;
}
long sgh_graphds_workload_top(void* g, uint32_t by, uint32_t k, float min_value, sgh_workload_edge* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadEdge> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadTop(by, k, min_value, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) { if (out) put_workload_edge(v[i], out + i); if (index) index[i] = idx[i]; }
    return n;
}
struct sgh_workload_vanished {
    uint64_t from_key, to_key; char from_uid[160], to_uid[160];
    double lat_mean, lat_dev, err_mean, err_dev; uint32_t n, last, row, pad;
};
long sgh_graphds_workload_vanished(void* g, sgh_workload_vanished* out, size_t cap) {
    std::vector<VanishedWorkload> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadVanished(&v);
    if (n < 0) return n;
    for (size_t i = 0; out && i < std::min(cap, v.size()); i++) {
        const VanishedWorkload& r = v[i]; sgh_workload_vanished& o = out[i];
        std::memset(&o, 0, sizeof o);
        o.from_key = r.FromKey; o.to_key = r.ToKey;
        std::strncpy(o.from_uid, r.FromUID.c_str(), sizeof o.from_uid - 1); std::strncpy(o.to_uid, r.ToUID.c_str(), sizeof o.to_uid - 1);
        o.lat_mean = r.LatMean; o.lat_dev = r.LatDev; o.err_mean = r.ErrMean; o.err_dev = r.ErrDev; o.n = r.N; o.last = r.Last; o.row = r.Row;
    }
    return n;
}
// the workload rows (K16): the two switches (a parameter 0 = its default), the last flushed window's workload rows (who each is,
// then the engine's sg_node_out), their trend rows (as sg_node_trend) and a selection over them
int sgh_graphds_set_workload_nodes(void* g, int on) { return static_cast<HostCtx*>(g)->ds->SetWorkloadNodes(on != 0); }
int sgh_graphds_set_workload_node_trend(void* g, uint32_t shift, uint32_t warmup, uint32_t ttl, uint64_t max_entries) {
    sg_trend_params p{}; p.struct_size = sizeof p; p.shift = shift; p.warmup = warmup; p.ttl = ttl; p.max_entries = max_entries;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadNodeTrend(p);
}
struct sgh_workload_node { char type[16]; char uid[160]; sg_node_out row; };
static_assert(sizeof(sgh_workload_node) == 16 + 160 + 136, "sgh_workload_node: the names, then sg_node_out");
static void put_workload_node(const WorkloadNode& r, sgh_workload_node* o) {
    std::memset(o, 0, sizeof *o);
    std::strncpy(o->type, r.Type.c_str(), sizeof o->type - 1); std::strncpy(o->uid, r.UID.c_str(), sizeof o->uid - 1);
    o->row = r.Row;
}
long sgh_graphds_workload_nodes(void* g, sgh_workload_node* out, size_t cap) {
    std::vector<WorkloadNode> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadNodes(&v);
    if (n < 0) return n;
    for (size_t i = 0; out && i < std::min(cap, v.size()); i++) put_workload_node(v[i], out + i);
    return n;
}
long sgh_graphds_workload_node_trends(void* g, sg_node_trend* out, size_t cap) {
    std::vector<sg_node_trend> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadNodeTrends(&v);
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_node_trend));
    return n;
}
long sgh_graphds_workload_nodes_top(void* g, uint32_t by, uint32_t k, float min_value, sgh_workload_node* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadNode> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadNodesTop(by, k, min_value, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) { if (out) put_workload_node(v[i], out + i); if (index) index[i] = idx[i]; }
    return n;
}
// the workload ranking (K17): the switch (on = 0: off; a parameter 0 = its default) and the selection over the last flushed window's
// rank rows — the workload rows as sgh_graphds_workload_nodes gives them, then each one's sg_node_rank
int sgh_graphds_set_workload_rank(void* g, int on, uint32_t iters, uint32_t damping_q8, uint32_t seed, float seed_min_score) {
    sg_rank_params p{}; p.struct_size = sizeof p; p.iters = iters; p.damping_q8 = damping_q8; p.seed = seed; p.seed_min_score = seed_min_score;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadRank(on ? &p : nullptr);
}
struct sgh_workload_culprit { sgh_workload_node node; sg_node_rank rank; };
static_assert(sizeof(sgh_workload_culprit) == 16 + 160 + 136 + 16, "sgh_workload_culprit: sgh_workload_node, then sg_node_rank");
long sgh_graphds_workload_culprits(void* g, uint32_t k, float min_share, sgh_workload_culprit* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadCulprit> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadCulprits(k, min_share, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) {
        if (out) { put_workload_node(v[i].Node, &out[i].node); out[i].rank = v[i].Rank; }
        if (index) index[i] = idx[i];
    }
    return n;
}
// the workload incidents (K18): the switch (on = 0: off) and the last flushed window's incident rows (sg_incident_out as the engine
// gives them) with the incident of every workload row
int sgh_graphds_set_workload_incidents(void* g, int on, uint32_t by, float min_value) {
    sg_incident_params p{}; p.struct_size = sizeof p; p.by = by; p.min_value = min_value;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadIncidents(on ? &p : nullptr);
}
long sgh_graphds_workload_incidents(void* g, sg_incident_out* out, size_t cap, uint32_t* node_incident, size_t node_cap, size_t* n_nodes) {
    std::vector<sg_incident_out> v; std::vector<uint32_t> ni;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadIncidents(&v, &ni);
    if (n < 0) return n;
    if (out && !v.empty()) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_incident_out));
    if (node_incident && !ni.empty()) std::memcpy(node_incident, ni.data(), std::min(node_cap, ni.size()) * sizeof(uint32_t));
    if (n_nodes) *n_nodes = ni.size();
    return n;
}
// the workload impact (K22): the switch (0, 0: off) and the last flushed window's incident rows with their impact rows
int sgh_graphds_set_workload_impact(void* g, uint32_t max_incidents, uint32_t max_hops) { return static_cast<HostCtx*>(g)->ds->SetWorkloadImpact(max_incidents, max_hops); }
long sgh_graphds_workload_impact(void* g, sg_incident_out* incidents, size_t inc_cap, size_t* n_incidents, uint64_t* impact, size_t cap_rows) {
    std::vector<sg_incident_out> v; std::vector<uint64_t> w;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadImpact(&v, &w);
    if (n < 0) return n;
    if (incidents && !v.empty()) std::memcpy(incidents, v.data(), std::min(inc_cap, v.size()) * sizeof(sg_incident_out));
    if (n_incidents) *n_incidents = v.size();
    if (impact && n) std::memcpy(impact, w.data(), std::min(cap_rows, (size_t)n) * SG_IMPACT_WORDS * sizeof(uint64_t));
    return n;
}
// the workload tracks (K19): the switch (on = 0: off) and the last flushed window's track rows and ended list as the engine gives them
int sgh_graphds_set_workload_tracks(void* g, int on, uint32_t quiet_windows, uint32_t max_tracks) {
    sg_track_params p{}; p.struct_size = sizeof p; p.quiet_windows = quiet_windows; p.max_tracks = max_tracks;
    return static_cast<HostCtx*>(g)->ds->SetWorkloadTracks(on ? &p : nullptr);
}
long sgh_graphds_workload_incident_tracks(void* g, sg_incident_track* out, size_t cap) {
    std::vector<sg_incident_track> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadIncidentTracks(&v);
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_incident_track));
    return n;
}
long sgh_graphds_workload_tracks_ended(void* g, sg_track_entry* out, size_t cap) {
    std::vector<sg_track_entry> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadTracksEnded(&v);
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_track_entry));
    return n;
}
// the latency percentiles (K20): the switch (spaces 0: off) and the last flushed window's quantiles in microseconds; which = 0 the
// node rows, 1 the group edges, 2 the workload rows; cap counts u32 words of out
int sgh_graphds_set_quantiles(void* g, uint32_t spaces, const uint32_t* permille, size_t n_q) {
    return static_cast<HostCtx*>(g)->ds->SetQuantiles(spaces, permille, n_q);
}
long sgh_graphds_latency(void* g, int which, const uint32_t* index, size_t n_index, uint32_t* out, size_t cap, size_t* words) {
    std::vector<uint32_t> v;
    GraphDS* ds = static_cast<HostCtx*>(g)->ds.get();
    const long n = which == 0 ? ds->NodeLatency(index, n_index, &v) : which == 1 ? ds->WorkloadEdgeLatency(index, n_index, &v)
                                                                                    : ds->WorkloadLatency(index, n_index, &v);
    if (words) *words = v.size();
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(uint32_t));
    return n;
}
// the tail baselines (K21): the switch (on = 0: off; a parameter 0 = its default), the last flushed window's tail rows — which = 0 the
// node rows and 2 the workload rows (sg_node_trend), 1 the group edges (sg_edge_trend); cap counts rows of out — and the selection
// over the workload rows by their tail rows, as sgh_graphds_workload_nodes_top gives it
int sgh_graphds_set_tail_trend(void* g, uint32_t spaces, uint32_t permille, int on, uint32_t shift, uint32_t warmup, uint32_t ttl, uint64_t max_entries) {
    sg_trend_params p{}; p.struct_size = sizeof p; p.shift = shift; p.warmup = warmup; p.ttl = ttl; p.max_entries = max_entries;
    return static_cast<HostCtx*>(g)->ds->SetTailTrend(spaces, permille, on ? &p : nullptr);
}
long sgh_graphds_tail_trends(void* g, int which, void* out, size_t cap) {
    GraphDS* ds = static_cast<HostCtx*>(g)->ds.get();
    if (which == 1) {
        std::vector<sg_edge_trend> v;
        const long n = ds->WorkloadEdgeTailTrends(&v);
        if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_edge_trend));
        return n;
    }
    std::vector<sg_node_trend> v;
    const long n = which == 0 ? ds->NodeTailTrends(&v) : ds->WorkloadTailTrends(&v);
    if (n > 0 && out) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(sg_node_trend));
    return n;
}
long sgh_graphds_workload_tail_top(void* g, uint32_t by, uint32_t k, float min_value, sgh_workload_node* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadNode> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadTailTop(by, k, min_value, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) { if (out) put_workload_node(v[i], out + i); if (index) index[i] = idx[i]; }
    return n;
}
// the traffic baselines (K23): the switch (on = 0: off; a parameter 0 = its default) and the selection over the workload rows by
// their traffic rows, as sgh_graphds_workload_nodes_top gives it
int sgh_graphds_set_traffic_trend(void* g, uint32_t spaces, int on, uint32_t shift, uint32_t warmup, uint32_t ttl, uint64_t max_entries,
                                  uint32_t rate_floor, uint64_t load_floor_ns) {
    sg_traffic_params p{}; p.struct_size = sizeof p; p.shift = shift; p.warmup = warmup; p.ttl = ttl; p.max_entries = max_entries;
    p.rate_floor = rate_floor; p.load_floor_ns = load_floor_ns;
    return static_cast<HostCtx*>(g)->ds->SetTrafficTrend(spaces, on ? &p : nullptr);
}
long sgh_graphds_workload_traffic_top(void* g, uint32_t by, uint32_t k, float min_value, sgh_workload_node* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadNode> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadTrafficTop(by, k, min_value, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) { if (out) put_workload_node(v[i], out + i); if (index) index[i] = idx[i]; }
    return n;
}
// the SLO burn rates (K24): the switch (on = 0: off), a workload's objective word by its owner UID, the SLO rows (SG_SLO_WORDS u64
// each; the count, min(count, cap) rows written) and the selection by a burn rate, as sgh_graphds_workload_nodes_top gives it
int sgh_graphds_set_slo(void* g, uint32_t spaces, int on, uint32_t latency_bin, uint32_t latency_target_ppm, uint32_t error_target_ppm,
                        uint32_t short_windows, uint32_t long_windows, uint32_t min_burn_q10, uint64_t min_requests) {
    sg_slo_params p{}; p.struct_size = sizeof p; p.latency_bin = latency_bin; p.latency_target_ppm = latency_target_ppm;
    p.error_target_ppm = error_target_ppm; p.short_windows = short_windows; p.long_windows = long_windows; p.min_burn_q10 = min_burn_q10;
    p.min_requests = min_requests;
    return static_cast<HostCtx*>(g)->ds->SetSLO(spaces, on ? &p : nullptr);
}
int sgh_graphds_set_workload_slo(void* g, const char* workload, uint32_t objective) {
    return static_cast<HostCtx*>(g)->ds->SetWorkloadSLO(workload ? workload : "", objective);
}
long sgh_graphds_workload_slo(void* g, uint64_t* out, size_t cap) {
    std::vector<uint64_t> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadSLO(&v);
    if (n < 0) return n;
    if (out) std::memcpy(out, v.data(), std::min(cap, (size_t)n) * SG_SLO_WORDS * sizeof(uint64_t));
    return n;
}
long sgh_graphds_workload_slo_top(void* g, uint32_t by, uint32_t k, uint32_t min_value_q10, sgh_workload_node* out, uint32_t* index, size_t cap) {
    std::vector<WorkloadNode> v; std::vector<uint32_t> idx;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadSLOTop(by, k, min_value_q10, &v, &idx);
    if (n < 0) return n;
    for (size_t i = 0; i < std::min(cap, v.size()); i++) { if (out) put_workload_node(v[i], out + i); if (index) index[i] = idx[i]; }
    return n;
}
// the replica outliers (K25): the switch (on = 0: off; a 0 among the parameters is the engine's default) and the selection — per
// selected pod its UID, its workload's owner UID, the two row indices, the flags and the words of the side `by` names
struct sgh_replica_outlier { char pod[160]; char workload[160]; uint32_t node_index, workload_index, flags; int32_t err_excess_q20;
                             uint32_t lat_ratio_q10, share_q10, tail_pod, tail_peers, replicas; };
static_assert(sizeof(sgh_replica_outlier) == 320 + 36, "sgh_replica_outlier: the names, then nine words");
int sgh_graphds_set_replica_outliers(void* g, int on, uint32_t min_replicas, uint64_t min_requests, uint32_t min_err_excess_q20, uint32_t min_lat_ratio_q10,
                                     uint32_t tail_permille, uint32_t min_tail_bins) {
    sg_replica_params p{}; p.struct_size = sizeof p; p.min_replicas = min_replicas; p.min_requests = min_requests; p.min_err_excess_q20 = min_err_excess_q20;
    p.min_lat_ratio_q10 = min_lat_ratio_q10; p.tail_permille = tail_permille; p.min_tail_bins = min_tail_bins;
    return static_cast<HostCtx*>(g)->ds->SetReplicaOutliers(on ? &p : nullptr);
}
long sgh_graphds_workload_replica_outliers(void* g, uint32_t by, uint32_t k, uint32_t min_value, sgh_replica_outlier* out, size_t cap) {
    std::vector<ReplicaOutlier> v;
    const long n = static_cast<HostCtx*>(g)->ds->WorkloadReplicaOutliers(by, k, min_value, &v);
    if (n < 0) return n;
    for (size_t i = 0; out && i < std::min(cap, v.size()); i++) {
        sgh_replica_outlier* o = out + i;
        std::memset(o, 0, sizeof *o);
        std::strncpy(o->pod, v[i].PodUID.c_str(), sizeof o->pod - 1); std::strncpy(o->workload, v[i].Workload.c_str(), sizeof o->workload - 1);
        o->node_index = v[i].NodeIndex; o->workload_index = v[i].WorkloadIndex; o->flags = v[i].Flags; o->err_excess_q20 = v[i].ErrExcessQ20;
        o->lat_ratio_q10 = v[i].LatRatioQ10; o->share_q10 = v[i].ShareQ10; o->tail_pod = v[i].TailPod; o->tail_peers = v[i].TailPeers; o->replicas = v[i].Replicas;
    }
    return n;
}
int sgh_graphds_ingest_wire(void* g, const uint8_t* recs, size_t n, const uint32_t* kafka_msgs) {
    return static_cast<HostCtx*>(g)->ds->IngestWire(recs, n, kafka_msgs);
}
int sgh_graphds_persist_request(void* g, int64_t start_ms, uint64_t latency, const char* from_ip, const char* from_type, const char* from_uid,
                                const char* to_ip, const char* to_type, const char* to_uid, const char* protocol, uint32_t status,
                                const char* method, int tls) {
    datastore::Request r; r.StartTime = start_ms; r.Latency = latency; r.FromIP = from_ip; r.FromType = from_type; r.FromUID = from_uid;
    r.ToIP = to_ip; r.ToType = to_type; r.ToUID = to_uid; r.Protocol = protocol; r.StatusCode = status; r.Method = method; r.Tls = tls != 0;
    return static_cast<HostCtx*>(g)->ds->PersistRequest(&r);
}
long sgh_graphds_flush(void* g, int64_t window_end_ms, sgh_edge_row* out, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    const long n = c->ds->FlushWindow(window_end_ms);
    if (n < 0) return n;
    const size_t m = std::min(cap, c->sink.rows.size());
    for (size_t i = 0; i < m; i++) {
        const EdgeRow& r = c->sink.rows[i]; sgh_edge_row& o = out[i];
        std::memset(&o, 0, sizeof o);
        std::strncpy(o.from_type, r.FromType.c_str(), sizeof o.from_type - 1); std::strncpy(o.to_type, r.ToType.c_str(), sizeof o.to_type - 1);
        std::strncpy(o.from_uid, r.FromUID.c_str(), sizeof o.from_uid - 1); std::strncpy(o.to_uid, r.ToUID.c_str(), sizeof o.to_uid - 1);
        o.count = r.Count; o.err_count = r.ErrCount; o.sum_ns = r.SumNs; o.max_ns = r.MaxNs; o.sumsq_us = r.SumSqUs; o.p50_us = r.P50Us; o.p99_us = r.P99Us;
        o.score = r.Score; o.lat_z = r.LatZ; o.err_ratio = r.ErrRatio; o.alive = r.Alive;
    }
    return n;
}
// ---- f-2: socket lines ----
struct sgh_sockinfo { uint32_t pid; uint64_t fd; uint32_t saddr; uint16_t sport; uint32_t daddr; uint16_t dport; };
void* sgh_sockline_create(uint32_t pid, uint64_t fd) { return new SocketLine(pid, fd); }
void sgh_sockline_destroy(void* l) { delete static_cast<SocketLine*>(l); }
void sgh_sockline_add(void* l, uint64_t ts, const sgh_sockinfo* si) {
    if (!si) { static_cast<SocketLine*>(l)->AddValue(ts, nullptr); return; }
    SockInfo s; s.Pid = si->pid; s.Fd = si->fd; s.Saddr = si->saddr; s.Sport = si->sport; s.Daddr = si->daddr; s.Dport = si->dport;
    static_cast<SocketLine*>(l)->AddValue(ts, &s);
}
int sgh_sockline_get(void* l, uint64_t ts, uint64_t now_ns, sgh_sockinfo* out) {
    SockInfo s; const SockErr e = static_cast<SocketLine*>(l)->GetValue(ts, now_ns, &s);
    if (e == SockErr::Ok && out) { out->pid = s.Pid; out->fd = s.Fd; out->saddr = s.Saddr; out->sport = s.Sport; out->daddr = s.Daddr; out->dport = s.Dport; }
    return (int)e;
}
// getConnectionInfo against `proc_root` (sock_num_line.go:399-429): 0 = seeded, else SocketLine::Seed
int sgh_sockline_seed(void* l, const char* proc_root, uint64_t now_kernel_ns) { return (int)static_cast<SocketLine*>(l)->SeedFromProc(proc_root, now_kernel_ns); }
int sgh_proc_inode_of_link(const char* link, char* inode, size_t cap) {
    std::string v;
    if (!procfs::InodeOfLink(link, &v) || v.size() + 1 > cap) return -1;
    std::memcpy(inode, v.c_str(), v.size() + 1);
    return 0;
}
int sgh_proc_parse_tcp_line(const char* line, uint32_t* laddr, uint16_t* lport, uint32_t* raddr, uint16_t* rport) {
    return procfs::ParseTcpLine(line, laddr, lport, raddr, rport) ? 0 : -1;
}
void sgh_sockline_delete_unused(void* l) { static_cast<SocketLine*>(l)->DeleteUnused(); }
size_t sgh_sockline_len(void* l) { return static_cast<SocketLine*>(l)->Size(); }
int sgh_sockline_at(void* l, size_t i, uint64_t* ts, uint64_t* last_match, sgh_sockinfo* out) {
    auto* sl = static_cast<SocketLine*>(l);
    if (i >= sl->Size()) return -1;
    const TimestampedSocket v = sl->At(i);
    if (ts) *ts = v.Timestamp;
    if (last_match) *last_match = v.LastMatch;
    if (out && v.Open) { out->pid = v.Info.Pid; out->fd = v.Info.Fd; out->saddr = v.Info.Saddr; out->sport = v.Info.Sport; out->daddr = v.Info.Daddr; out->dport = v.Info.Dport; }
    return v.Open ? 1 : 0;
}
// TCP connect records (BpfTcpEvent, 64 bytes each) through processTcpConnect; returns values added
size_t sgh_graphds_tcp_wire(void* g, const uint8_t* recs, size_t n) {
    auto* c = static_cast<HostCtx*>(g); size_t added = 0;
    for (size_t i = 0; i < n; i++) {
        const tcp_state::TcpConnectEvent e = tcp_state::DecodeWire(recs + i * tcp_state::kWireSize);
        const bool ok = c->conns.ProcessTcpConnect(e);
        if (ok && e.Type == tcp_state::kClosed) c->ds->ConnClosed(e.Pid, e.Fd);     // data.go:484-494
        added += ok ? 1 : 0;
    }
    return added;
}
// process exec / exit (proc events, data.go:354-377) and the HTTP/2 minute sweep (:553-567)
void sgh_graphds_proc_exec(void* g, uint32_t pid) { static_cast<HostCtx*>(g)->ds->ProcExec(pid); }
void sgh_graphds_proc_exit(void* g, uint32_t pid) { auto* c = static_cast<HostCtx*>(g); c->conns.ClearProc(pid); c->ds->ProcExit(pid); }   // clearProc first, data.go:364
// new socket lines are seeded from `root` (NULL or "" = off); the seeded value is stamped first_kernel − (first_user − now_user)
void sgh_graphds_set_proc_root(void* g, const char* root, uint64_t first_kernel_ns, uint64_t first_user_ns, uint64_t now_user_ns) {
    static_cast<HostCtx*>(g)->conns.SetProcRoot(root ? root : "", first_kernel_ns, first_user_ns, now_user_ns);
}
size_t sgh_graphds_pg_statements(void* g) { return static_cast<HostCtx*>(g)->ds->Packer().PgStatements(); }
void sgh_graphds_seed_stats(void* g, uint64_t out[2]) { auto* c = static_cast<HostCtx*>(g); out[0] = c->conns.SeedsOk(); out[1] = c->conns.SeedsFailed(); }
void sgh_graphds_sweep_http2(void* g) { static_cast<HostCtx*>(g)->ds->SweepHttp2(); }
// counters of the assembler: [0] streams pending, [1] parsers, [2] dropped: pid not live, [3] dropped: method/path unparsed, [4] dropped: time
void sgh_graphds_http2_stats(void* g, uint64_t out[5]) {
    const Http2Assembler& a = static_cast<HostCtx*>(g)->ds->Packer().Http2();
    out[0] = a.Pending(); out[1] = a.Parsers(); out[2] = a.DroppedNotLive(); out[3] = a.DroppedUnparsed(); out[4] = a.DroppedTime();
}

// ---- stand-alone HPACK decoder / HTTP/2 assembler (known-answer and differential tests) ----
void* sgh_hpack_create(uint32_t max_table) { return new hpack::Decoder(max_table); }
void sgh_hpack_destroy(void* d) { delete static_cast<hpack::Decoder*>(d); }
// decodes `block`; the emitted fields are appended to buf as name\0value\0 (lengths in lens[2*i], lens[2*i+1]).
// returns the number of fields, or -(1 + fields emitted before the error) on a decoding error
long sgh_hpack_write(void* d, const uint8_t* block, size_t n, char* buf, size_t cap, uint32_t* lens, size_t max_fields) {
    auto* dec = static_cast<hpack::Decoder*>(d);
    size_t used = 0, nf = 0;
    dec->SetEmitFunc([&](std::string_view name, std::string_view value) {
        if (nf < max_fields && used + name.size() + value.size() <= cap) {
            std::memcpy(buf + used, name.data(), name.size()); used += name.size();
            std::memcpy(buf + used, value.data(), value.size()); used += value.size();
            lens[2 * nf] = (uint32_t)name.size(); lens[2 * nf + 1] = (uint32_t)value.size();
        }
        nf++;
    });
    const bool ok = dec->Write(block, n);
    dec->SetEmitFunc(nullptr);
    return ok ? (long)nf : -(long)(1 + nf);
}
size_t sgh_hpack_table_len(void* d) { return static_cast<hpack::Decoder*>(d)->DynamicTableLen(); }
uint32_t sgh_hpack_table_size(void* d) { return static_cast<hpack::Decoder*>(d)->DynamicTableSize(); }
size_t sgh_hpack_table_at(void* d, size_t i, char* buf, size_t cap, uint32_t lens[2]) {
    const hpack::HeaderField& f = static_cast<hpack::Decoder*>(d)->DynamicTableAt(i);
    lens[0] = (uint32_t)f.Name.size(); lens[1] = (uint32_t)f.Value.size();
    if (f.Name.size() + f.Value.size() > cap) return 0;
    std::memcpy(buf, f.Name.data(), f.Name.size()); std::memcpy(buf + f.Name.size(), f.Value.data(), f.Value.size());
    return f.Name.size() + f.Value.size();
}
long sgh_huffman_decode(const uint8_t* p, size_t n, char* out, size_t cap) {
    std::string s; if (!hpack::HuffmanDecode(p, n, &s)) return -1;
    if (s.size() > cap) return -2;
    std::memcpy(out, s.data(), s.size()); return (long)s.size();
}
long sgh_huffman_encode(const char* p, size_t n, char* out, size_t cap) {
    std::string s; hpack::HuffmanEncode(std::string(p, n), &s);
    if (s.size() > cap) return -2;
    std::memcpy(out, s.data(), s.size()); return (long)s.size();
}
uint32_t sgh_go_atoi_u32(const char* p, size_t n) { return GoAtoiU32(std::string_view(p, n)); }

struct sgh_h2_out { char method[64]; char path[1100]; char authority[160]; char protocol[8]; uint32_t status_code; uint64_t latency; };
void* sgh_h2_create(void) { return new Http2Assembler(); }
void sgh_h2_destroy(void* a) { delete static_cast<Http2Assembler*>(a); }
int sgh_h2_event(void* a, uint32_t pid, uint64_t fd, int method_id, const uint8_t* payload, uint32_t size, uint64_t write_ns, int tls, sgh_h2_out* out) {
    l7_req::L7Event e; e.Pid = pid; e.Fd = fd; e.ProtocolId = l7_req::BPF_L7_PROTOCOL_HTTP2; e.MethodId = (uint8_t)method_id;
    e.PayloadSize = size > l7_req::kMaxPayload ? (uint32_t)l7_req::kMaxPayload : size; std::memcpy(e.Payload, payload, e.PayloadSize);
    e.WriteTimeNs = write_ns; e.Tls = tls != 0;
    Http2Request r;
    if (!static_cast<Http2Assembler*>(a)->OnEvent(e, &r)) return 0;
    auto put = [](char* dst, size_t cap, const std::string& s) { const size_t n = s.size() < cap - 1 ? s.size() : cap - 1; std::memcpy(dst, s.data(), n); dst[n] = 0; };
    std::memset(out, 0, sizeof *out);
    put(out->method, sizeof out->method, r.Method); put(out->path, sizeof out->path, r.Path); put(out->authority, sizeof out->authority, r.Authority);
    put(out->protocol, sizeof out->protocol, r.Protocol); out->status_code = r.StatusCode; out->latency = r.Latency;
    return 1;
}
void sgh_h2_proc_exec(void* a, uint32_t pid) { static_cast<Http2Assembler*>(a)->ProcExec(pid); }
void sgh_h2_proc_exit(void* a, uint32_t pid) { static_cast<Http2Assembler*>(a)->ProcExit(pid); }
void sgh_h2_conn_closed(void* a, uint32_t pid, uint64_t fd) { static_cast<Http2Assembler*>(a)->ConnClosed(pid, fd); }
void sgh_h2_sweep(void* a) { static_cast<Http2Assembler*>(a)->Sweep(); }
size_t sgh_h2_pending(void* a) { return static_cast<Http2Assembler*>(a)->Pending(); }
size_t sgh_h2_parsers(void* a) { return static_cast<Http2Assembler*>(a)->Parsers(); }
// ---- edge egress (edges_payload.hpp, f-3) ----
// the rows of the last sgh_graphds_flush as "/edges/" payloads of at most `batch` rows, concatenated with '\n' into buf;
// returns the number of payloads (0 when the window had no edge), or -(bytes needed) when buf is too small
long sgh_graphds_edges_json(void* g, const char* monitoring_id, const char* idem_key, const char* node_id, const char* version, size_t batch,
                            char* buf, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    std::string all; long n = 0;
    JsonEdgeSink sink(PayloadMetadata{monitoring_id ? monitoring_id : "", idem_key ? idem_key : "", node_id ? node_id : "", version ? version : ""}, batch,
                      [&](const char*, const std::string& body) { if (n) all.push_back('\n'); all += body; n++; return 0; });
    sink.PersistEdges(c->sink.window_end, c->sink.rows);
    if (all.size() + 1 > cap) return -(long)(all.size() + 1);
    std::memcpy(buf, all.data(), all.size()); buf[all.size()] = 0;
    return n;
}
// the same encoder over caller-supplied rows (tests)
long sgh_edges_json_from_rows(const sgh_edge_row* in, size_t n_rows, int64_t window_end_ms, const char* monitoring_id, const char* idem_key, const char* node_id,
                              const char* version, size_t batch, char* buf, size_t cap) {
    std::vector<EdgeRow> rows(n_rows);
    for (size_t i = 0; i < n_rows; i++) {
        EdgeRow& r = rows[i]; const sgh_edge_row& o = in[i];
        r.FromType = o.from_type; r.FromUID = o.from_uid; r.ToType = o.to_type; r.ToUID = o.to_uid;
        r.Count = o.count; r.ErrCount = o.err_count; r.SumNs = o.sum_ns; r.MaxNs = o.max_ns; r.SumSqUs = o.sumsq_us; r.P50Us = o.p50_us; r.P99Us = o.p99_us;
        r.Score = o.score; r.LatZ = o.lat_z; r.ErrRatio = o.err_ratio; r.Alive = o.alive;
    }
    std::string all; long n = 0;
    JsonEdgeSink sink(PayloadMetadata{monitoring_id ? monitoring_id : "", idem_key ? idem_key : "", node_id ? node_id : "", version ? version : ""}, batch,
                      [&](const char*, const std::string& body) { if (n) all.push_back('\n'); all += body; n++; return 0; });
    sink.PersistEdges(window_end_ms, rows);
    if (all.size() + 1 > cap) return -(long)(all.size() + 1);
    std::memcpy(buf, all.data(), all.size()); buf[all.size()] = 0;
    return n;
}
size_t sgh_json_string(const char* s, size_t n, char* out, size_t cap) {
    std::string o; AppendJsonString(std::string(s, n), &o);
    if (o.size() + 1 <= cap) { std::memcpy(out, o.data(), o.size()); out[o.size()] = 0; }
    return o.size();
}

// ---- Kafka payload decode (kafka.hpp) ----
void sgh_packer_kafka_decode(void* p, int on) { static_cast<L7Packer*>(p)->SetKafkaDecode(on != 0); }
void sgh_graphds_kafka_decode(void* g, int on) { static_cast<HostCtx*>(g)->ds->SetKafkaDecode(on != 0); }
// decodes one payload; messages are serialised into buf as [u32 topic_n][i32 partition][u32 key_n][u32 value_n] topic key value ...
// returns the message count (also when buf is too small: then nothing is written), *status = kafka::Status
long sgh_kafka_decode(const uint8_t* payload, size_t size, int method_id, int api_version, int* status, uint8_t* buf, size_t cap) {
    std::vector<kafka::Message> msgs; size_t counted = 0, counted_only = 0;
    const kafka::Status st = kafka::DecodePayload(payload, size, method_id, (int16_t)api_version, &msgs, &counted);
    const kafka::Status st2 = kafka::DecodePayload(payload, size, method_id, (int16_t)api_version, nullptr, &counted_only);   // the packer's mode
    if (st2 != st || counted != msgs.size() || counted_only != counted) { if (status) *status = 99; return -1; }           // self-check of the two modes
    if (status) *status = (int)st;
    size_t need = 0;
    for (const auto& m : msgs) need += 16 + m.Topic.size() + m.Key.size() + m.Value.size();
    if (need <= cap) {
        uint8_t* w = buf;
        for (const auto& m : msgs) {
            const uint32_t h[4] = {(uint32_t)m.Topic.size(), (uint32_t)m.Partition, (uint32_t)m.Key.size(), (uint32_t)m.Value.size()};
            std::memcpy(w, h, 16); w += 16;
            std::memcpy(w, m.Topic.data(), m.Topic.size()); w += m.Topic.size();
            std::memcpy(w, m.Key.data(), m.Key.size()); w += m.Key.size();
            std::memcpy(w, m.Value.data(), m.Value.size()); w += m.Value.size();
        }
    }
    return (long)msgs.size();
}
long sgh_kafka_decompress(int codec, const uint8_t* src, size_t n, uint8_t* out, size_t cap) {
    std::string s; if (!kafka::Decompress(codec, src, n, &s)) return -1;
    if (s.size() > cap) return -2;
    std::memcpy(out, s.data(), s.size()); return (long)s.size();
}
uint32_t sgh_crc32(int castagnoli, const uint8_t* p, size_t n) { return kafka::Crc32(p, n, castagnoli != 0); }
uint32_t sgh_xxh32(const uint8_t* p, size_t n, uint32_t seed) { return kafka::XXH32(p, n, seed); }
// the stand-alone packer's assembler
void sgh_packer_proc_exec(void* p, uint32_t pid) { static_cast<L7Packer*>(p)->Http2().ProcExec(pid); }
void sgh_packer_proc_exit(void* p, uint32_t pid) { static_cast<L7Packer*>(p)->ProcExit(pid); }
void sgh_packer_conn_closed(void* p, uint32_t pid, uint64_t fd) { static_cast<L7Packer*>(p)->ConnClosed(pid, fd); }
size_t sgh_packer_pg_statements(void* p) { return static_cast<L7Packer*>(p)->PgStatements(); }
size_t sgh_graphds_socklines(void* g) { return static_cast<HostCtx*>(g)->conns.Lines(); }
// An OWNING reference to the line of (pid, fd), or null: sgh_graphds_proc_exit -> ClearProc(pid) drops the tracker's reference, and a
// wrapper that still looks at the line must not be left with freed memory.  sgh_sockline_ref_get is the SocketLine* the
// sgh_sockline_* calls take, valid until sgh_sockline_ref_release.
void* sgh_graphds_sockline(void* g, uint32_t pid, uint64_t fd) {
    auto sp = static_cast<HostCtx*>(g)->conns.Share(pid, fd);
    return sp ? new std::shared_ptr<SocketLine>(std::move(sp)) : nullptr;
}
void* sgh_sockline_ref_get(void* ref) { return ref ? static_cast<std::shared_ptr<SocketLine>*>(ref)->get() : nullptr; }
void sgh_sockline_ref_release(void* ref) { delete static_cast<std::shared_ptr<SocketLine>*>(ref); }
// one clearSocketLines tick: open connections -> GraphDS::PersistAliveConnection (-> SG_EV_ALIVE records)
size_t sgh_graphds_sweep(void* g, int64_t now_ms, int send_alive) { auto* c = static_cast<HostCtx*>(g); return c->conns.Sweep(now_ms, send_alive != 0, c->ds.get()); }

size_t sgh_graphds_labels(void* g, char* buf, size_t cap) { return join_labels(static_cast<HostCtx*>(g)->ds->Labels(), buf, cap); }
uint64_t sgh_graphds_dropped_parse(void* g) { return static_cast<HostCtx*>(g)->ds->Packer().DroppedParse(); }
int sgh_graphds_set_selection(void* g, uint32_t k, float min_score) { return static_cast<HostCtx*>(g)->ds->SetSelection(k, min_score); }
void sgh_graphds_clear_selection(void* g) { static_cast<HostCtx*>(g)->ds->ClearSelection(); }
size_t sgh_graphds_sink_rows(void* g) { return static_cast<HostCtx*>(g)->sink.rows.size(); }   // rows the last sgh_graphds_flush handed to the sink
void* sgh_graphds_engine(void* g) { return static_cast<HostCtx*>(g)->h; }
// {events offered, batches dropped, engine errors, live node ids, requests / kafka events / alive connections / pods / services that reached the inner store}
void sgh_graphds_counters(void* g, uint64_t out[9]) {
    auto* c = static_cast<HostCtx*>(g);
    out[0] = c->ds->EventsOffered(); out[1] = c->ds->BatchesDropped(); out[2] = c->ds->EngineErrors(); out[3] = c->ds->LiveIds();
    out[4] = c->inner.requests; out[5] = c->inner.kafka; out[6] = c->inner.alive; out[7] = c->inner.pods; out[8] = c->inner.services;
}
// mock inspection
size_t sgh_mock_events(void* g, sg_event* out, size_t cap) {
    auto* c = static_cast<HostCtx*>(g); if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    const size_t k = std::min(cap, m->events.size()); if (k) std::memcpy(out, m->events.data(), k * sizeof(sg_event));
    return m->events.size();
}
size_t sgh_mock_table_ops(void* g, uint32_t* out3, size_t cap) {
    auto* c = static_cast<HostCtx*>(g); if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    const size_t k = std::min(cap, m->table_ops.size());
    for (size_t i = 0; i < k; i++) { out3[3 * i] = m->table_ops[i][0]; out3[3 * i + 1] = m->table_ops[i][1]; out3[3 * i + 2] = m->table_ops[i][2]; }
    return m->table_ops.size();
}
// the stand-in's flush counts {flush_window calls, flush_window_top calls, last k} and the last min_score
void sgh_mock_flushes(void* g, uint32_t out[3], float* min_score) {
    auto* c = static_cast<HostCtx*>(g); out[0] = out[1] = out[2] = 0; if (min_score) *min_score = 0;
    if (!c->mock) return;
    auto* m = reinterpret_cast<MockEngine*>(c->h); std::lock_guard<std::mutex> l(m->mu);
    out[0] = m->flushes; out[1] = m->top_flushes; out[2] = m->top_k; if (min_score) *min_score = m->top_min;
}
size_t sgh_mock_k15_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k15_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k15_ops[i].data(), 32);
    return m->k15_ops.size();
}
size_t sgh_mock_k16_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k16_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k16_ops[i].data(), 32);
    return m->k16_ops.size();
}
size_t sgh_mock_k17_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k17_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k17_ops[i].data(), 32);
    return m->k17_ops.size();
}
size_t sgh_mock_k18_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k18_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k18_ops[i].data(), 32);
    return m->k18_ops.size();
}
size_t sgh_mock_k22_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k22_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k22_ops[i].data(), 32);
    return m->k22_ops.size();
}
size_t sgh_mock_k21_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k21_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k21_ops[i].data(), 32);
    return m->k21_ops.size();
}
size_t sgh_mock_k23_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k23_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k23_ops[i].data(), 32);
    return m->k23_ops.size();
}
size_t sgh_mock_k25_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k25_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k25_ops[i].data(), 32);
    return m->k25_ops.size();
}
size_t sgh_mock_k24_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k24_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k24_ops[i].data(), 32);
    return m->k24_ops.size();
}
size_t sgh_mock_k20_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k20_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k20_ops[i].data(), 32);
    return m->k20_ops.size();
}
size_t sgh_mock_k19_ops(void* g, uint64_t* out4, size_t cap) {
    auto* c = static_cast<HostCtx*>(g);
    if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h);
    std::lock_guard<std::mutex> lk(m->mu);
    for (size_t i = 0; i < std::min(cap, m->k19_ops.size()); i++) std::memcpy(out4 + 4 * i, m->k19_ops[i].data(), 32);
    return m->k19_ops.size();
}
size_t sgh_mock_group_ops(void* g, uint32_t* out2, size_t cap) {
    auto* c = static_cast<HostCtx*>(g); if (!c->mock) return 0;
    auto* m = reinterpret_cast<MockEngine*>(c->h); std::lock_guard<std::mutex> l(m->mu);
    const size_t k = std::min(cap, m->group_ops.size());
    for (size_t i = 0; i < k; i++) { out2[2 * i] = m->group_ops[i][0]; out2[2 * i + 1] = m->group_ops[i][1]; }
    return m->group_ops.size();
}
uint32_t sgh_mock_label_count(void* g) { auto* c = static_cast<HostCtx*>(g); return c->mock ? reinterpret_cast<MockEngine*>(c->h)->label_count : 0; }

}  // extern "C"

// ---- the sharded window sequence with caller-supplied stages and collectives (alaz_amd/csrc/shard_seq.hpp) ------------------
// The engine library runs the very same function with its HIP stages and RCCL (sg_window_run_sharded); exported here so that
// the sequence can be driven without a GPU: tests/test_sharded.py plugs the numpy stand-in backend and gloo collectives in.
#include "../shard_seq.hpp"
extern "C" int sgh_run_sharded_window(const sg_shard_stages* stages, const sg_shard_comm* comm) { return sg_run_sharded_window(stages, comm); }

// ---- synthetic capture for the streaming harness (tools/c5_stream.py) ---------------------------------------------------------
// BASELINE config 5 is a STREAM of raw l7_event records over a 20 M-edge graph.  A ring of distinct 1096-byte records large enough
// to touch millions of edges per window would be tens of GB; instead the harness keeps a ring of PACKED events (32 bytes each,
// drawn from the seeded edge list by alaz_amd/replay.py) and this feeder expands every one of them into the wire record the
// reference's perf reader would have seen — the same fields and payloads replay.to_wire() writes (ebpf/l7_req/l7.go:345-369;
// "GET /user HTTP1.1" + Host header, a Postgres simple query, count-only Kafka) — in a thread-local buffer, 256 records at a
// time, and hands them to GraphDS::IngestWire: payload parse, label interning, packing and batching all run as in production.
// Paced: the caller's share of `rate` events/s since *t0 (steady_clock ns); returns the events fed, stops when *stop != 0.
#include <atomic>
#include <chrono>
#include <thread>
extern "C" long sgh_graphds_feed_expanded(void* g, const sg_event* ring, size_t ring_n, size_t first, size_t stride_chunks, size_t chunk,
                                          const char* const* labels, size_t n_labels, double rate_per_s, const int64_t* t0_ns, const volatile int* stop,
                                          volatile long* fed_out) {
    auto* ctx = static_cast<HostCtx*>(g);
    constexpr size_t kRec = l7_req::kWireSize, kBatch = 256;
    std::vector<uint8_t> buf(kBatch * kRec);
    static const char kPg[] = "SELECT * FROM users WHERE id = 1";
    long fed = 0;
    size_t pos = first;
    auto now_ns = [] { return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    while (!*stop) {
        const double ahead = (double)fed - rate_per_s * (double)(now_ns() - *t0_ns) * 1e-9;
        if (ahead > 0) { std::this_thread::sleep_for(std::chrono::microseconds((long)std::min(2000.0, ahead / rate_per_s * 1e6 + 1.0))); continue; }
        const size_t n_chunk = std::min(chunk, ring_n - pos);
        for (size_t i0 = 0; i0 < n_chunk; i0 += kBatch) {
            const size_t nb = std::min(kBatch, n_chunk - i0);
            for (size_t i = 0; i < nb; i++) {
                const sg_event& e = ring[pos + i0 + i];
                uint8_t* r = buf.data() + i * kRec;
                std::memset(r, 0, 36); std::memset(r + 1060, 0, kRec - 1060);
                const uint64_t fd = 3 + (pos + i0 + i) % 97; const uint32_t pid = 4242, status = e.status;
                std::memcpy(r, &fd, 8); std::memcpy(r + 8, &e.write_time_ns, 8); std::memcpy(r + 16, &pid, 4); std::memcpy(r + 20, &status, 4);
                std::memcpy(r + 24, &e.duration_ns, 8);
                r[32] = e.protocol;
                uint32_t pl = 0;
                char* p = reinterpret_cast<char*>(r + 36);
                if (e.protocol == SG_PROTO_HTTP) {
                    r[33] = 1;                                                          // GET (ebpf/l7_req/l7.go method enum)
                    const bool external = e.daddr >= 0x08080001u && e.daddr < 0x08090001u;
                    if (e.host_label && e.host_label <= n_labels) pl = (uint32_t)std::snprintf(p, 1024, "GET /user HTTP1.1\r\nHost: %s\r\nAccept: */*\r\n\r\n", labels[e.host_label - 1]);
                    else if (external) pl = (uint32_t)std::snprintf(p, 1024, "GET /user HTTP1.1\r\nAccept: */*\r\n\r\n");
                    else pl = (uint32_t)std::snprintf(p, 1024, "GET /user HTTP1.1\r\nHost: svc.cluster.local\r\nAccept: */*\r\n\r\n");
                } else if (e.protocol == SG_PROTO_POSTGRES) {
                    r[33] = 2;                                                          // SIMPLE_QUERY
                    const uint32_t len = (uint32_t)sizeof kPg + 4;                      // query + NUL + the length word
                    p[0] = 'Q'; p[1] = (char)(len >> 24); p[2] = (char)(len >> 16); p[3] = (char)(len >> 8); p[4] = (char)len;
                    std::memcpy(p + 5, kPg, sizeof kPg); pl = 5 + (uint32_t)sizeof kPg;
                } else if (e.protocol == SG_PROTO_KAFKA) r[33] = (e.flags & SG_EV_CONSUME) ? 2 : 1;
                std::memcpy(r + 1060, &pl, 4); r[1064] = 1; r[1066] = (e.flags & SG_EV_TLS) ? 1 : 0;
                const uint16_t sport = (uint16_t)(32768 + (pos + i0 + i) % 28232), dport = e.protocol == SG_PROTO_POSTGRES ? 5432 : (e.protocol == SG_PROTO_KAFKA ? 9092 : 80);
                std::memcpy(r + 1076, &e.saddr, 4); std::memcpy(r + 1080, &sport, 2); std::memcpy(r + 1084, &e.daddr, 4); std::memcpy(r + 1088, &dport, 2);
            }
            ctx->ds->IngestWire(buf.data(), nb, nullptr);
            fed += (long)nb;
        }
        if (fed_out) *fed_out = fed;
        pos += stride_chunks * chunk;
        if (pos >= ring_n) pos = first;
    }
    if (fed_out) *fed_out = fed;
    return fed;
}
