// CPU driver of alaz_amd/csrc/sg_plan.hpp (tests/plan_driver.py builds and runs it):  plan_driver <stage>  reads the stage's cases
// from stdin, one per line (empty lines and lines that begin with # are skipped), and prints one JSON object per case.
//
//   g++ -O2 -std=c++17 -Wall -Werror -o plan_driver tests/micro/plan_driver.cpp
//
// The engine-level stages (plan, pair, k5_form, k5_efeat, k3_forms, prepare_fold) take `name key=value ...` (plan_json.hpp: parse_case);
// the window stages take the numbers their comment lists, in that order.  plan --knobs prints the knob names, one per line;
// plan --domains and pair --domains print the kernel instantiations the library holds, per family, as lists of template arguments.
// An unknown stage is exit status 2, with the stages on stderr.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../alaz_amd/csrc/join_host.hpp"
#include "plan_json.hpp"

using namespace sgplan;
typedef unsigned long long ull;

// ---------------------------------------------------------------------------------------------------------- engine-level stages

// the engine's plan of a case, as sg_create makes it
struct Planned { Case cs; sg_config cfg; Plan p; std::string why; int rc; };

static Planned plan_case(const std::string& line) {
    Planned P;
    DeviceFacts dev;
    P.cs = parse_case(line, dev);
    P.rc = check_config(P.cs.c, &P.cfg);
    if (P.rc == SG_OK) P.rc = make_plan(P.cfg, dev, P.cs.ov, &P.p, &P.why);
    return P;
}
// a stage that takes no keys of its own
static bool refuse_rest(const Case& cs) {
    if (!cs.rest.empty()) std::fprintf(stderr, "unknown key %s\n", cs.rest[0].first.c_str());
    return !cs.rest.empty();
}
// l1= / l2=: the join tables' level-1 entries and level-2 bytes; false for any other key
static bool take_tables(const Case& cs, u64* l1, u64* l2, bool* given) {
    for (const auto& kv : cs.rest) {
        if (kv.first == "l1") *l1 = kv.second; else if (kv.first == "l2") *l2 = kv.second;
        else { std::fprintf(stderr, "unknown key %s\n", kv.first.c_str()); return false; }
        *given = true;
    }
    return true;
}
// the join tables as sg_create builds them
struct Tables { sgjoin::Layout L{}; sgjoin::Table jt; std::vector<u32> mirror; };
static void init_tables(Tables& t, const sg_config& cfg, const Plan& p) {
    t.L = sgjoin::Table::make_layout(cfg.max_ips, cfg.max_known_nodes, p.max_blocks);
    t.mirror.assign(t.L.words, 0);
    t.jt.init(t.L, t.mirror.data(), p.variant == 0);
}

template <size_t N, size_t M>
static void put_keys(Json& j, const char* name, const std::array<Key<N>, M>& keys) {
    j.arr(name);
    for (const Key<N>& key : keys) { j.arr(); for (const int v : key) j.kv(nullptr, v); j.end(); }
    j.end();
}

// Dev's scalar fields (alaz_amd/csrc/sg_device.h), zero as at create
struct DevScalars {
    u32 ipmask, ipmask2, jl1mask, jl2_words, ck_n, jstage_bytes, jl2_in_lds, max_known, max_labels, max_obip, rank, world, emask, obmask;
    u64 max_edges;
    u32 variant, np, nwg, ss, sa, pslots, k1a_ct, narrow, nb, pb, rb, k1b_split, npb, sn, sw, punits, k1b_ht, hist, agg_slots, ovf_cap, pcap,
        batch_state, ablate, k2_sortw, k1a_rot, k1a_ticket_base, alive_cap, warm, kept_compact, dh_g, dh_ppw, dh_ns, hub_cap, ncap, layers;
};

static void put_pass_a(Json& j, const char* key, u32 l1, size_t l2, const PassA& a) {
    j.obj(key);
    j.kv("l1_entries", l1); j.kv("l2_bytes", l2);
    PUT(a, l2_u16); PUT(a, k1a_nsub); PUT(a, k1a_team); PUT(a, k1a_teams); PUT(a, k1a_nt); PUT(a, k1a_ct); PUT(a, l2_in_lds); PUT(a, k1a_lds);
    j.end();
}

static void put_kernels(Json& j, const char* key, const Kernels& k) {
    j.obj(key);
    j.kv("k1a_family", k.k1a.family); j.kv("k1a_l2", k.k1a.l2); j.kv("k1a_sharded", k.k1a.sharded); j.kv("k1a_hist", k.k1a.hist);
    j.kv("k1a_nsub", k.k1a.nsub); j.kv("k1a_pb", k.k1a.pb);
    PUT(k, k1b_family); PUT(k, k1b_u); PUT(k, k1b_spt); PUT(k, k1b_pack); PUT(k, k1b_hist); PUT(k, k1b_share); PUT(k, k1b_warm);
    PUT(k, k2_dh); PUT(k, k4_split); PUT(k, k4_mfma); PUT(k, k5_mfma);
    j.end();
}

// plan: the plan, the Dev fields the engine fills from it at create, pass A for the join tables as sg_create builds them and, given
// l1 / l2, pass A for those sizes; "kernels" (and "kernels_after") is the kernel instantiation each launch site takes under that plan
static int stage_plan(const std::string& line) {
    Planned P = plan_case(line);
    const Plan& p = P.p; const sg_config& cfg = P.cfg;
    u64 l1 = 0, l2 = 0; bool after = false;
    if (!take_tables(P.cs, &l1, &l2, &after)) return 2;
    int rc = P.rc;
    PassA pa; Tables t;
    if (rc == SG_OK) {                                          // pass A is planned for the tables' initial state
        init_tables(t, cfg, p);
        if (p.variant == 0 && !plan_pass_a(p, t.jt.l1_entries, t.jt.blocks_bytes(), P.cs.ov, &pa)) rc = SG_ENOSPC;
    }
    Json j;
    j.str("name", P.cs.name).kv("rc", rc);
    if (rc == SG_OK) {
        DevScalars d{};
        plan_to_dev(p, cfg, d);
        d.ipmask = t.L.ipcap - 1; d.ipmask2 = t.L.ip2cap - 1;
        j.kv("cus", p.cus);
        j.obj("plan");
#define P_(x) PUT(p, x)
#define D_(x) PUT(d, x)
        D_(variant); D_(narrow); D_(hist); D_(agg_slots); D_(nb); D_(np); D_(pb); D_(nwg); D_(k1b_split); D_(k1b_ht); D_(npb); D_(rb); D_(pcap); D_(sa);
        D_(sn); D_(sw); D_(punits); D_(ss); D_(pslots); D_(ovf_cap); D_(warm); P_(k1b_threads); P_(k1b_u); P_(k1b_pack); P_(k1b_lds);
        P_(ecap); P_(obcap); P_(ob_list_cap); D_(ncap); D_(alive_cap); D_(hub_cap); P_(max_blocks);
        P_(k3_ranges); P_(k3_slices); P_(k3in_lds); D_(k2_sortw); D_(dh_g); D_(dh_ppw); D_(dh_ns);
        P_(k4_split); P_(k5_grid); P_(k3_fuse_allowed); P_(k6_one_wg); P_(use_mfma);
        P_(k1b_order); P_(k1_grid); P_(n_copy); P_(n_stage); P_(arena_on); P_(n_slots); D_(ablate);
        D_(ipmask); D_(ipmask2); D_(jl1mask); D_(jl2_words); D_(ck_n); D_(jstage_bytes); D_(jl2_in_lds); D_(max_known); D_(max_labels); D_(max_obip);
        D_(rank); D_(world); D_(emask); D_(obmask); D_(max_edges); D_(k1a_ct); D_(batch_state); D_(k1a_rot); D_(k1a_ticket_base); D_(kept_compact);
        D_(layers);
#undef P_
#undef D_
        j.end();
        put_pass_a(j, "pass_a", t.jt.l1_entries, t.jt.blocks_bytes(), pa);
        Kernels kn = choose_kernels(p, pa, cfg);
        put_kernels(j, "kernels", kn);
        if (after) {
            PassA pb = pa;                                      // (the engine keeps its geometry when the tables leave no legal one)
            const bool ok = p.variant != 0 || plan_pass_a(p, (u32)l1, (size_t)l2, P.cs.ov, &pb);
            j.kv("upsert_rc", ok ? SG_OK : SG_ENOSPC);
            put_pass_a(j, "pass_a_after", (u32)l1, (size_t)l2, pb);
            kn.k1a = choose_pass_a(p, pb, cfg);                // (the rest of the choice is made once, at create)
            put_kernels(j, "kernels_after", kn);
        }
    }
    j.emit();
    return 0;
}

// pair: pass A's tile pairs (PassA::k1a_pair, PassAKernel::pair) — what the LDS layout of k1a_team_partition is made of, pass A's
// choice and the kernel key it leads to; l1= / l2= as in plan, by default the tables as sg_create builds them
static int stage_pair(const std::string& line) {
    Planned P = plan_case(line);
    const Plan& p = P.p;
    u64 l1 = 0, l2 = 0; bool given = false;
    if (!take_tables(P.cs, &l1, &l2, &given)) return 2;
    int rc = P.rc;
    PassA pa;
    if (rc == SG_OK) {
        if (!given) { Tables t; init_tables(t, P.cfg, p); l1 = t.jt.l1_entries; l2 = t.jt.blocks_bytes(); }
        if (p.variant != 0 || !plan_pass_a(p, (u32)l1, (size_t)l2, P.cs.ov, &pa)) rc = SG_ENOSPC;
    }
    Json j;
    j.str("name", P.cs.name).kv("rc", rc);
    if (rc == SG_OK) {
        const PassAKernel k = choose_pass_a(p, pa, P.cfg);
        PUT(p, np); PUT(p, nb); PUT(p, narrow); j.kv("l1_entries", l1); j.kv("l2_bytes", l2);
        PUT(pa, l2_u16); PUT(pa, l2_in_lds); PUT(pa, k1a_team); PUT(pa, k1a_teams); PUT(pa, k1a_nt); PUT(pa, k1a_ct); PUT(pa, k1a_lds); PUT(pa, k1a_pair);
        PUT(pa, k1a_pair_lds); j.kv("lds_cap", kLdsBytes); j.kv("pair_default", kK1aPairDefault);
        j.obj("kernel"); PUT(k, family); PUT(k, l2); PUT(k, sharded); PUT(k, pb); PUT(k, pair); j.end();
    }
    j.emit();
    return 0;
}

// k5_form: k5_edge_score's form (Plan::k5_form / k5_grid, Kernels::k5_form) — make_plan's return code and message, the form, its grid
// and the constants the grid is derived from
static int stage_k5_form(const std::string& line) {
    const Planned P = plan_case(line);
    if (refuse_rest(P.cs)) return 2;
    Json j;
    j.str("name", P.cs.name).kv("rc", P.rc).str("why", P.why);
    if (P.rc == SG_OK) {
        const Kernels k = choose_kernels(P.p, PassA{}, P.cfg);
        PUT(P.p, k5_form); PUT(P.p, k5_grid); j.kv("kernel_form", k.k5_form); PUT(P.p, cus); PUT(P.p, ncap); PUT(P.cfg, max_edges);
        j.kv("form_default", k5_form_default(P.cfg)); j.kv("lanes_min_edges", kK5LanesMinEdges); j.kv("lanes_wg_lds", kK5LanesWgLds);
        j.kv("lanes_waves", kK5LanesWaves); j.kv("lds_cap", kLdsBytes);
    }
    j.emit();
    return 0;
}

// k5_efeat: where the edge features are computed (Plan::k5_efeat, Kernels::k5_efeat, SG_K5_EFEAT) — the form, its grid and the
// features' place as the plan and the kernel choice have it, and the default
static int stage_k5_efeat(const std::string& line) {
    const Planned P = plan_case(line);
    if (refuse_rest(P.cs)) return 2;
    Json j;
    j.str("name", P.cs.name).kv("rc", P.rc).str("why", P.why);
    if (P.rc == SG_OK) {
        const Kernels k = choose_kernels(P.p, PassA{}, P.cfg);
        PUT(P.p, k5_form); PUT(P.p, k5_efeat); PUT(P.p, k5_grid); j.kv("kernel_form", k.k5_form); j.kv("kernel_efeat", k.k5_efeat);
        j.kv("form_default", k5_form_default(P.cfg)); j.kv("efeat_default", kK5EfeatDefault ? 1 : 0);
    }
    j.emit();
    return 0;
}

// k3_forms: K3's two batched-load forms (Plan::k3_in_form / k3_feat_lanes, Kernels likewise, SG_K3_IN_FORM / SG_K3_FEAT_LANES) — as the
// plan and the kernel choice have them, what they hang on (k5_form, k5_efeat, the slices) and the defaults
static int stage_k3_forms(const std::string& line) {
    const Planned P = plan_case(line);
    if (refuse_rest(P.cs)) return 2;
    Json j;
    j.str("name", P.cs.name).kv("rc", P.rc).str("why", P.why);
    if (P.rc == SG_OK) {
        const Kernels k = choose_kernels(P.p, PassA{}, P.cfg);
        PUT(P.p, k3_in_form); PUT(P.p, k3_feat_lanes); j.kv("kernel_in_form", k.k3_in_form); j.kv("kernel_feat_lanes", k.k3_feat_lanes);
        PUT(P.p, k5_form); PUT(P.p, k5_efeat); PUT(P.p, k3_slices); PUT(P.p, k3_ranges); j.kv("in_form_default", k3_in_form_default(P.cfg));
        j.kv("in_form_on", kK3InFormDefault ? 1 : 0); j.kv("feat_lanes_on", kK3FeatLanesDefault ? 1 : 0);
    }
    j.emit();
    return 0;
}

// prepare_fold: which window closes launch no kc_prepare (Plan::prepare_fold, close_folds) — the plan's choice, the facts it rests on,
// and close_folds for every (the close keeps state, the host tries the warm path, outbound-IP mode) a close can come with
static int stage_prepare_fold(const std::string& line) {
    const Planned P = plan_case(line);
    if (refuse_rest(P.cs)) return 2;
    const Plan& p = P.p;
    Json j;
    j.str("name", P.cs.name).kv("rc", P.rc);
    if (P.rc == SG_OK) {
        PUT(p, prepare_fold); PUT(p, warm); PUT(p, narrow); PUT(p, variant); PUT(p, k1b_threads); PUT(p, k1b_lds); j.kv("prepare_lds", kPrepareLds);
        j.arr("closes");
        for (int warm = 0; warm < 2; warm++) for (int wt = 0; wt < 2; wt++) for (u32 ob = 0; ob < 3; ob++)
            j.list<u32>(nullptr, {(u32)warm, (u32)wt, ob, close_folds(p, warm != 0, wt != 0, ob) ? 1u : 0u});
        j.end();
    }
    j.emit();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- window stages

// the numbers of a line, in order; what the line does not hold reads as zero
struct Numbers {
    std::istringstream in;
    explicit Numbers(const std::string& line) : in(line) {}
    ull operator()() { ull v = 0; in >> v; return in ? v : 0; }
};

static sg_trend_params read_trend_params(Numbers& n) {     // struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved
    sg_trend_params p{};
    p.struct_size = (u32)n(); p.shift = (u32)n(); p.warmup = (u32)n(); p.ttl = (u32)n(); p.max_entries = n(); p.lat_floor_ns = n();
    p.err_floor = (u32)n(); p.reserved = (u32)n();
    return p;
}
// what every baseline's plan prints: the walk parameters check_* resolved, plan_*trend of them, the block's and one buffer's layout
static void put_trend(Json& j, const sg_trend_params& r, const TrendPlan& t) {
    PUT(r, shift); PUT(r, warmup); PUT(r, ttl); PUT(r, max_entries);
    PUT(t, entries); PUT(t, wgs); PUT(t, soa_bytes); PUT(t, ctl_bytes); PUT(t, blk_bytes); PUT(t, thread_bytes); PUT(t, rows_bytes); PUT(t, total_bytes);
    j.kv("per_thread", kTrendPerThread);
    j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}}).put_layout("soa_layout", t.soa_layout);
}
static void put_trend_limits(Json& j, const sg_trend_params& r) {
    PUT(r, lat_floor_ns); PUT(r, err_floor); j.kv("threads", kTrendThreads); j.kv("max_wgs", kTrendMaxWgs);
}
// a vanished list's resolved parameters and plan_vanished of them
static void put_vanished(Json& j, const sg_vanished_params& r, const VanishedPlan& v) {
    PUT(r, silent_windows); PUT(r, min_seen); PUT(r, max_rows); PUT(v, rows); PUT(v, total_bytes);
    j.put_layout("layout", v.layout).put_slot(v.slot, {{"list", v.slot_list}, {"count", v.slot_count}});
}

static void put_select(Json& j, const char* key, const SelPlan& s) {
    j.obj(key);
    PUT(s, wgs); PUT(s, key_bytes); PUT(s, hist_bytes); PUT(s, blk_bytes); PUT(s, pair_bytes); PUT(s, state_bytes); PUT(s, scratch_bytes); PUT(s, stage_rows);
    j.end();
}
// select  "max_edges": plan_select(max_edges, used = true / false), the scratch's layout, the node selection's block over max_edges
// node rows with a counter block of kCtrBytes (plan_node_select) and k7_sort's LDS at SG_SELECT_MAX_K
static int stage_select(const std::string& line) {
    constexpr u64 kCtrBytes = 200;        // any size that is no multiple of 256: the engine passes its own counter block's
    const u64 me = std::stoull(line);
    Json j;
    j.kv("max_edges", me);
    put_select(j, "used", plan_select(me, true));
    put_select(j, "unused", plan_select(me, false));
    j.put_layout("layout", plan_select(me, true).layout);
    const NodeSelPlan n = plan_node_select((u32)me, kCtrBytes);
    j.obj("node");
    j.kv("ctr_in", kCtrBytes); j.kv("sel_scratch_bytes", n.sel.scratch_bytes); PUT(n, sel_off); PUT(n, total_bytes);
    j.put_layout("layout", n.layout).put_layout("sel_layout", n.sel.layout);
    j.end();
    j.kv("sort_lds_max_k", select_sort_lds(SG_SELECT_MAX_K)); j.kv("sort_lds_1", select_sort_lds(1)); j.kv("lds_bytes", kLdsBytes);
    j.kv("max_k", (unsigned)SG_SELECT_MAX_K); j.kv("threads", kSelThreads); j.kv("max_wgs", kSelMaxWgs); j.kv("rows_per_wg", kSelRowsPerWg);
    j.emit();
    return 0;
}

// trend  "max_edges slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved": check_trend's verdict, the
// parameters it resolved and plan_trend of them
static int stage_trend(const std::string& line) {
    Numbers n(line);
    const ull me = n(), slots = n();
    const sg_trend_params p = read_trend_params(n);
    sg_trend_params r{};
    const int rc = check_trend(p, me, &r);
    Json j;
    j.kv("max_edges", me).kv("slots", slots).kv("rc", rc);
    j.kv("params_size", sizeof(sg_trend_params)).kv("edge_trend_size", sizeof(sg_edge_trend)).kv("entry_size", sizeof(sg_trend_entry));
    if (rc == SG_OK) { put_trend(j, r, plan_trend(me, (u32)slots, r)); put_trend_limits(j, r); }
    j.emit();
    return 0;
}

// vanish  "max_edges slots warmup ttl max_entries struct_size silent_windows min_seen max_rows": check_vanished's verdict against the
// trend those parameters resolve to, the parameters it resolved and plan_vanished of them
static int stage_vanish(const std::string& line) {
    Numbers n(line);
    const ull me = n(), slots = n();
    sg_trend_params tp{};
    tp.struct_size = (u32)sizeof(sg_trend_params); tp.warmup = (u32)n(); tp.ttl = (u32)n(); tp.max_entries = n();
    sg_vanished_params p{};
    p.struct_size = (u32)n(); p.silent_windows = (u32)n(); p.min_seen = (u32)n(); p.max_rows = (u32)n();
    sg_trend_params tr{};
    Json j;
    if (check_trend(tp, me, &tr) != SG_OK) { j.kv("trend_rc", -1).emit(); return 0; }
    const TrendPlan t = plan_trend(me, (u32)slots, tr);
    sg_vanished_params r{};
    const int rc = check_vanished(p, tr, &r);
    j.kv("max_edges", me).kv("slots", slots).kv("rc", rc).kv("params_size", sizeof(sg_vanished_params)).kv("vanished_size", sizeof(sg_edge_vanished));
    PUT(tr, ttl); PUT(tr, warmup); PUT(t, entries); PUT(t, wgs);
    if (rc == SG_OK) {
        const VanishedPlan v = plan_vanished(t, (u32)slots, r);
        put_vanished(j, r, v);
        PUT(v, thread_bytes); PUT(v, blk_bytes); PUT(v, list_bytes); PUT(v, count_bytes); j.kv("threads", kTrendThreads);
    }
    j.emit();
    return 0;
}

// what plan_nodes and plan_group_nodes share
static void put_nodes(Json& j, const NodesPlan& n) {
    PUT(n, out_wgs); PUT(n, ranges); PUT(n, slices); PUT(n, node_wgs); PUT(n, node_per); PUT(n, dst_bytes); PUT(n, table_bytes); PUT(n, part_bytes);
    PUT(n, blk_bytes); PUT(n, rows_bytes); PUT(n, count_bytes); PUT(n, lds_bytes); PUT(n, total_bytes); j.kv("max_wgs", kNodesMaxWgs);
    j.put_layout("layout", n.layout).put_slot(n.slot, {{"rows", n.slot_rows}, {"count", n.slot_count}});
}
// nodes  "max_edges ncap slots": plan_nodes of it and the constants it plans with
static int stage_nodes(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), slots = in();
    const NodesPlan n = plan_nodes(me, (u32)ncap, (u32)slots);
    Json j;
    j.kv("max_edges", me); PUT(n, ncap); j.kv("slots", slots).kv("node_size", sizeof(sg_node_out));
    put_nodes(j, n);
    j.kv("threads", kNodesThreads).kv("chunk", kNodesChunk).kv("range_nodes", kNodesRangeNodes).kv("max_slices", kNodesMaxSlices);
    j.kv("side_bytes", kNodesSideBytes);
    j.emit();
    return 0;
}

// node_trend  "ncap slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved": check_node_trend's verdict, the
// parameters it resolved and plan_node_trend of them
static int stage_node_trend(const std::string& line) {
    Numbers n(line);
    const ull nc = n(), slots = n();
    const sg_trend_params p = read_trend_params(n);
    sg_trend_params r{};
    const int rc = check_node_trend(p, (u32)nc, &r);
    Json j;
    j.kv("ncap", nc).kv("slots", slots).kv("rc", rc).kv("node_trend_size", sizeof(sg_node_trend));
    if (rc == SG_OK) { put_trend(j, r, plan_node_trend((u32)nc, (u32)slots, r)); put_trend_limits(j, r); }
    j.emit();
    return 0;
}

static sg_rank_params read_rank_params(Numbers& n) {       // struct_size iters damping_q8 seed reserved
    sg_rank_params p{};
    p.struct_size = (u32)n(); p.iters = (u32)n(); p.damping_q8 = (u32)n(); p.seed = (u32)n(); p.reserved = (u32)n();
    return p;
}
// rank  "max_edges ncap slots struct_size iters damping_q8 seed reserved": check_rank's verdict, the parameters it resolved and plan_rank
static int stage_rank(const std::string& line) {
    Numbers n(line);
    const ull me = n(), nc = n(), slots = n();
    const sg_rank_params p = read_rank_params(n);
    sg_rank_params r{};
    const int rc = check_rank(p, &r);
    Json j;
    j.kv("max_edges", me).kv("ncap", nc).kv("slots", slots).kv("rc", rc).kv("rank_size", sizeof(sg_node_rank)).kv("params_size", sizeof(sg_rank_params));
    if (rc == SG_OK) {
        const RankPlan t = plan_rank(me, (u32)nc, (u32)slots);
        PUT(r, iters); PUT(r, damping_q8); PUT(r, seed); PUT(t, ranges); PUT(t, slices); PUT(t, prep_wgs); PUT(t, node_wgs); PUT(t, row_bytes);
        PUT(t, node_bytes); PUT(t, part_bytes); PUT(t, seed_bytes); PUT(t, stage_bytes); PUT(t, stage_idx_bytes); PUT(t, rows_bytes); PUT(t, lds_bytes);
        PUT(t, total_bytes);
        j.kv("range_nodes", kRankRangeNodes).kv("max_wgs", kRankMaxWgs).kv("max_edge_wgs", kRankMaxEdgeWgs).kv("lds_limit", kLdsBytes);
        j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}});
    }
    j.emit();
    return 0;
}

static sg_incident_params read_incident_params(Numbers& n) {   // struct_size by reserved
    sg_incident_params p{};
    p.struct_size = (u32)n(); p.by = (u32)n(); p.min_value = 0.5f; p.reserved = (u32)n();
    return p;
}
// incident  "max_edges ncap slots struct_size by reserved": check_incidents' verdict and plan_incidents
static int stage_incident(const std::string& line) {
    Numbers n(line);
    const ull me = n(), nc = n(), slots = n();
    const sg_incident_params p = read_incident_params(n);
    sg_incident_params r{};
    const int rc = check_incidents(p, &r);
    Json j;
    j.kv("max_edges", me).kv("ncap", nc).kv("slots", slots).kv("rc", rc).kv("out_size", sizeof(sg_incident_out)).kv("params_size", sizeof(sg_incident_params));
    if (rc == SG_OK) {
        const IncidentPlan t = plan_incidents(me, (u32)nc, (u32)slots);
        PUT(r, by); PUT(r, min_value); PUT(t, node_wgs); PUT(t, node_per); PUT(t, grid_wgs); PUT(t, hook_wgs); PUT(t, row_wgs); PUT(t, key_bytes);
        PUT(t, keys_bytes); PUT(t, blk_bytes); PUT(t, stage_bytes); PUT(t, rows_bytes); PUT(t, count_bytes); PUT(t, node_inc_bytes); PUT(t, total_bytes);
        j.kv("threads", kIncThreads).kv("max_wgs", kIncMaxWgs).kv("max_row_wgs", kIncMaxRowWgs);
        j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"node_inc", t.slot_node_inc}});
    }
    j.emit();
    return 0;
}

static sg_track_params read_track_params(Numbers& n) {     // struct_size quiet_windows max_tracks reserved
    sg_track_params p{};
    p.struct_size = (u32)n(); p.quiet_windows = (u32)n(); p.max_tracks = (u32)n(); p.reserved = (u32)n();
    return p;
}
// what plan_tracks and plan_group_tracks share
static void put_tracks(Json& j, const sg_track_params& r, const TrackPlan& t) {
    j.kv("quiet", r.quiet_windows);
    PUT(t, max_tracks); PUT(t, anchors); PUT(t, wgs); PUT(t, per); PUT(t, init_wgs); PUT(t, node_wgs); PUT(t, fold_wgs); PUT(t, member_bytes);
    PUT(t, table_bytes); PUT(t, state_bytes); PUT(t, inc_bytes); PUT(t, claim_bytes); PUT(t, blk_bytes); PUT(t, rows_bytes); PUT(t, ended_bytes);
    PUT(t, count_bytes); PUT(t, total_bytes);
    j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}, {"ended", t.slot_ended}, {"ended_count", t.slot_count}});
}
// track  "max_known max_labels ncap slots struct_size quiet_windows max_tracks reserved": check_tracks' verdict and plan_tracks
static int stage_track(const std::string& line) {
    Numbers n(line);
    const ull mk = n(), ml = n(), nc = n(), slots = n();
    const sg_track_params p = read_track_params(n);
    sg_track_params r{};
    const int rc = check_tracks(p, (u32)nc, &r);
    Json j;
    j.kv("max_known", mk).kv("max_labels", ml).kv("ncap", nc).kv("slots", slots).kv("rc", rc).kv("row_size", sizeof(sg_incident_track));
    j.kv("entry_size", sizeof(sg_track_entry)).kv("params_size", sizeof(sg_track_params)).kv("stats_size", sizeof(sg_track_stats));
    if (rc == SG_OK) {
        put_tracks(j, r, plan_tracks((u32)mk, (u32)ml, (u32)nc, r.max_tracks, (u32)slots));
        j.kv("fold_rounds", kTrkFoldRounds).kv("threads", kTrkThreads).kv("max_wgs", kTrkMaxWgs);
    }
    j.emit();
    return 0;
}

// group  "max_edges max_known ncap max_groups slots world struct_size reserved0 reserved1": check_groups' verdict and plan_groups
static int stage_group(const std::string& line) {
    Numbers n(line);
    const ull me = n(), mk = n(), nc = n(), mg = n(), slots = n(), world = n();
    sg_group_params p{};
    p.struct_size = (u32)n(); p.max_groups = (u32)mg; p.reserved[0] = (u32)n(); p.reserved[1] = (u32)n();
    sg_group_params r{};
    const int rc = check_groups(p, (u32)mk, (u32)world, &r);
    Json j;
    j.kv("max_edges", me).kv("max_known", mk).kv("ncap", nc).kv("slots", slots).kv("rc", rc).kv("edge_size", sizeof(sg_group_edge));
    j.kv("params_size", sizeof(sg_group_params));
    if (rc == SG_OK) {
        const GroupPlan t = plan_groups(me, (u32)mk, (u32)nc, r.max_groups, (u32)slots);
        PUT(t, max_groups); PUT(t, gk); PUT(t, kb); PUT(t, key_bytes); PUT(t, passes); PUT(t, tiles); PUT(t, key_wgs); PUT(t, chunks); PUT(t, cpw);
        PUT(t, heads_wgs); PUT(t, stitch_wgs); PUT(t, keys_bytes); PUT(t, idx_bytes); PUT(t, map_bytes); PUT(t, hist_bytes); PUT(t, chunkcnt_bytes);
        PUT(t, part_bytes); PUT(t, meta_bytes); PUT(t, blk_bytes); PUT(t, stage_bytes); PUT(t, rows_bytes); PUT(t, count_bytes); PUT(t, total_bytes);
        j.kv("tile", kGrpTile).kv("chunk", kGrpChunk).kv("max_wgs", kGrpMaxWgs);
        j.put_layout("layout", t.layout);
        j.put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"row_group", t.slot_row_group}, {"perm", t.slot_perm}});
    }
    j.emit();
    return 0;
}

// group_trend  "max_edges slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved vstruct_size silent_windows
// min_seen max_rows counter_bytes": check_group_trend's verdict, the parameters it resolved and plan_group_trend of them; as "van"
// check_vanished's verdict against them and plan_vanished over that plan; as "sel" plan_group_select(max_edges, counter_bytes)
static int stage_group_trend(const std::string& line) {
    Numbers n(line);
    const ull me = n(), slots = n();
    const sg_trend_params p = read_trend_params(n);
    sg_vanished_params vp{};
    vp.struct_size = (u32)n(); vp.silent_windows = (u32)n(); vp.min_seen = (u32)n(); vp.max_rows = (u32)n();
    const ull cb = n();
    sg_trend_params r{};
    const int rc = check_group_trend(p, me, &r);
    Json j;
    j.kv("max_edges", me).kv("slots", slots).kv("rc", rc).kv("trend_size", sizeof(sg_edge_trend)).kv("group_edge_size", sizeof(sg_group_edge));
    if (rc == SG_OK) {
        const GroupTrendPlan t = plan_group_trend(me, (u32)slots, r);
        put_trend(j, r, t); put_trend_limits(j, r);
        sg_vanished_params vr{};
        const int vrc = check_vanished(vp, r, &vr);
        j.obj("van").kv("rc", vrc).kv("slots", slots);
        if (vrc == SG_OK) put_vanished(j, vr, plan_vanished(t, (u32)slots, vr));
        j.end();
    }
    const GroupSelPlan g = plan_group_select(me, cb);
    j.obj("sel").kv("slots", 1).kv("wgs", g.sel.wgs).kv("stage_rows", g.stage_rows).kv("scratch_bytes", g.sel.scratch_bytes);
    j.kv("key_bytes", g.sel.key_bytes).kv("total_bytes", g.total_bytes).kv("select_max_k", SG_SELECT_MAX_K);
    j.put_layout("layout", g.layout).put_layout("k7_layout", g.sel.layout);
    j.end();
    j.emit();
    return 0;
}

// group_nodes  "max_edges ncap max_groups slots max_entries counter_bytes": check_group_nodes' verdict and plan_group_nodes; as
// "trend" check_group_node_trend's verdict over default parameters with that max_entries and plan_group_node_trend; as "sel"
// plan_group_node_select(NC, counter_bytes)
static int stage_group_nodes(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), mg = in(), slots = in(), maxe = in(), cb = in();
    const int rc = check_group_nodes((u32)mg, (u32)ncap);
    Json j;
    j.kv("max_edges", me).kv("ncap", ncap).kv("max_groups", mg).kv("slots", slots).kv("rc", rc).kv("node_size", sizeof(sg_node_out));
    j.kv("node_trend_size", sizeof(sg_node_trend));
    if (rc == SG_OK) {
        const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
        PUT(n, gk); PUT(n, nc);
        put_nodes(j, n);
        j.kv("lds_limit", kLdsBytes);
        sg_trend_params p{};
        p.struct_size = sizeof(sg_trend_params); p.max_entries = maxe;
        sg_trend_params r{};
        const int trc = check_group_node_trend(p, n.nc, &r);
        j.obj("trend").kv("rc", trc).kv("slots", slots);
        if (trc == SG_OK) {
            const GroupNodeTrendPlan t = plan_group_node_trend(n.nc, (u32)slots, r);
            PUT(r, max_entries); PUT(t, entries); PUT(t, wgs); PUT(t, soa_bytes); PUT(t, rows_bytes); PUT(t, total_bytes); j.kv("per_thread", kTrendPerThread);
            j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}}).put_layout("soa_layout", t.soa_layout);
        }
        j.end();
        const NodeSelPlan g = plan_group_node_select(n.nc, cb);
        j.obj("sel").kv("slots", 1).kv("wgs", g.sel.wgs).kv("scratch_bytes", g.sel.scratch_bytes).kv("key_bytes", g.sel.key_bytes);
        j.kv("total_bytes", g.total_bytes).put_layout("layout", g.layout).put_layout("k7_layout", g.sel.layout);
        j.end();
    }
    j.emit();
    return 0;
}

// group_rank  "max_edges ncap max_groups slots rows struct_size iters damping_q8 seed reserved": check_rank's verdict, the parameters
// it resolved, plan_group_rank over plan_group_nodes' row capacity and key count, and the workgroups of k17_edge that work on a
// window of `rows` workload rows
static int stage_group_rank(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), mg = in(), slots = in(), rows = in();
    const sg_rank_params p = read_rank_params(in);
    sg_rank_params r{};
    const int rc = check_rank(p, &r);
    Json j;
    j.kv("max_edges", me).kv("ncap", ncap).kv("max_groups", mg).kv("slots", slots).kv("rc", rc).kv("rank_size", sizeof(sg_node_rank));
    j.kv("params_size", sizeof(sg_rank_params));
    if (rc == SG_OK) {
        const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
        const GroupRankPlan t = plan_group_rank(me, n.nc, n.gk, (u32)slots);
        PUT(r, iters); PUT(r, damping_q8); PUT(r, seed); PUT(t, nc); PUT(t, gk); PUT(t, ranges); PUT(t, slices); PUT(t, pos_wgs); PUT(t, prep_wgs);
        PUT(t, node_wgs); PUT(t, pos_bytes); PUT(t, edge_bytes); PUT(t, w_bytes); PUT(t, node_bytes); PUT(t, part_bytes); PUT(t, seed_bytes);
        PUT(t, stage_bytes); PUT(t, stage_idx_bytes); PUT(t, rows_bytes); PUT(t, lds_bytes); PUT(t, total_bytes);
        j.kv("range_rows", kGrpRankRangeRows).kv("slice_edges", kGrpRankSliceEdges).kv("max_slices", kGrpRankMaxSlices).kv("max_wgs", kGrpRankMaxWgs);
        j.kv("part_budget", kGrpRankPartBudget).kv("lds_limit", kLdsBytes).kv("live_wgs", group_rank_live_wgs(t, rows));
        j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}});
    }
    j.emit();
    return 0;
}

// group_incident  "max_edges ncap max_groups slots rows group_edges struct_size by reserved": check_incidents' verdict,
// plan_group_incidents over plan_group_nodes' row capacity and key count, and what one workgroup of each folding pass strides over
// in a window of `rows` workload rows and `group_edges` group edges
static int stage_group_incident(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), mg = in(), slots = in(), rows = in(), ge = in();
    const sg_incident_params p = read_incident_params(in);
    sg_incident_params r{};
    const int rc = check_incidents(p, &r);
    Json j;
    j.kv("max_edges", me).kv("ncap", ncap).kv("max_groups", mg).kv("slots", slots).kv("rc", rc).kv("out_size", sizeof(sg_incident_out));
    j.kv("params_size", sizeof(sg_incident_params));
    if (rc == SG_OK) {
        const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
        const GroupIncidentPlan t = plan_group_incidents(me, n.nc, n.gk, (u32)slots);
        PUT(r, by); PUT(t, nc); PUT(t, gk); PUT(t, node_wgs); PUT(t, node_per); PUT(t, grid_wgs); PUT(t, fold_wgs); PUT(t, hook_wgs); PUT(t, row_wgs);
        PUT(t, pos_bytes); PUT(t, node_bytes); PUT(t, esrc_bytes); PUT(t, keys_bytes); PUT(t, blk_bytes); PUT(t, stage_bytes); PUT(t, rows_bytes);
        PUT(t, count_bytes); PUT(t, node_inc_bytes); PUT(t, total_bytes);
        j.kv("threads", kGrpIncThreads).kv("max_wgs", kGrpIncMaxWgs).kv("max_row_wgs", kGrpIncMaxRowWgs).kv("fold_rounds", kGrpIncFoldRounds);
        j.kv("table_slots", kGrpIncSlots).kv("fold_rows", group_incident_fold_rows(t, rows)).kv("row_edges", group_incident_row_edges(t, ge));
        j.put_layout("layout", t.layout).put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"node_inc", t.slot_node_inc}});
    }
    j.emit();
    return 0;
}

// group_track  "max_groups max_known max_labels nc slots struct_size quiet_windows max_tracks reserved": check_tracks' verdict over nc
// and plan_group_tracks
static int stage_group_track(const std::string& line) {
    Numbers n(line);
    const ull mg = n(), mk = n(), ml = n(), nc = n(), slots = n();
    const sg_track_params p = read_track_params(n);
    sg_track_params r{};
    const int rc = check_tracks(p, (u32)nc, &r);
    Json j;
    j.kv("max_groups", mg).kv("max_known", mk).kv("max_labels", ml).kv("nc", nc).kv("slots", slots).kv("rc", rc);
    if (rc == SG_OK) {
        const TrackPlan t = plan_group_tracks((u32)mg, (u32)mk, (u32)ml, (u32)nc, r.max_tracks, (u32)slots);
        put_tracks(j, r, t);
        PUT(t, ncap);
    }
    j.emit();
    return 0;
}

// group_impact  "max_edges ncap max_groups slots max_incidents max_hops": check_group_impact's verdict and plan_group_impact over
// plan_group_nodes' row capacity and key count
static int stage_group_impact(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), mg = in(), slots = in(), mi = in(), mh = in();
    const int rc = (mi > 0xFFFFFFFFull || mh > 0xFFFFFFFFull) ? SG_EINVAL : check_group_impact((u32)mi, (u32)mh);
    Json j;
    j.kv("max_edges", me).kv("ncap", ncap).kv("max_groups", mg).kv("slots", slots).kv("max_incidents", mi).kv("max_hops", mh).kv("rc", rc);
    j.kv("impact_words", SG_IMPACT_WORDS).kv("limit_incidents", SG_IMPACT_MAX_INCIDENTS).kv("limit_hops", SG_IMPACT_MAX_HOPS);
    if (rc == SG_OK) {
        const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
        const GroupImpactPlan t = plan_group_impact(me, n.nc, n.gk, (u32)slots, (u32)mi);
        PUT(t, nc); PUT(t, gk); PUT(t, words); PUT(t, node_wgs); PUT(t, edge_wgs); PUT(t, finish_wgs); j.kv("launches", 2 * mh + 4);
        PUT(t, pos_bytes); PUT(t, mask_bytes); PUT(t, ends_bytes); PUT(t, node_bytes); PUT(t, cnt_bytes); PUT(t, rows_bytes); PUT(t, count_bytes);
        PUT(t, total_bytes); j.kv("threads", kImpThreads).kv("max_wgs", kImpMaxWgs);
        j.put_layout("layout", t.layout);
        j.put_slot(t.slot, {{"mask", t.slot_mask}, {"rows", t.slot_rows}, {"hops", t.slot_hops}, {"count", t.slot_count}});
    }
    j.emit();
    return 0;
}

// quantile  "max_edges ncap max_groups slots spaces world n_q q0 .. q(n_q - 1)": check_quantiles' and check_quantile_keys' verdicts,
// then plan_quantiles over plan_group_nodes' key count and row capacity: per space its grids, sizes, layout and slot region
static int stage_quantile(const std::string& line) {
    Numbers in(line);
    const ull me = in(), ncap = in(), mg = in(), slots = in(), spaces = in(), world = in(), nq = in();
    u32 qm[64] = {}, out[SG_Q_MAX] = {}, n_out = 0;
    for (ull k = 0; k < nq && k < 64; k++) qm[k] = (u32)in();
    const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
    int rc = check_quantiles((u32)spaces, qm, nq, (u32)world, out, &n_out);
    if (rc == SG_OK) rc = check_quantile_keys((u32)spaces, (u32)ncap, n.gk);
    Json j;
    j.kv("max_edges", me).kv("ncap", ncap).kv("slots", slots).kv("spaces", spaces).kv("rc", rc).kv("n_q", n_out);
    j.arr("permille");
    for (u32 k = 0; k < n_out; k++) j.kv(nullptr, out[k]);
    j.end();
    if (rc == SG_OK) {
        const QuantPlan q = plan_quantiles(me, (u32)ncap, n.gk, n.nc, (u32)spaces, (u32)slots);
        PUT(n, nc); PUT(n, gk); PUT(q, tgt_bytes); PUT(q, group_slot_bytes); PUT(q, lds_bytes); PUT(q, total_bytes);
        j.kv("fold_threads", kQFoldThreads).kv("range", kQRange).kv("max_wgs", kQMaxWgs).kv("q_max", kQMax);
        j.arr("space");
        for (int k = 0; k < 3; k++) {
            const QuantSpace& s = q.sp[k];
            j.obj().kv("on", s.on ? 1 : 0);
            if (s.on) {
                PUT(s, cap); PUT(s, sides); j.list("sorted", {s.sorted.ranges, s.sorted.slices}); j.list("scattered", {s.scattered.ranges, s.scattered.slices});
                PUT(s, finish_wgs); PUT(s, pos_wgs); PUT(s, tgt_wgs); PUT(s, pos_bytes); PUT(s, part_bytes); PUT(s, hist_bytes); PUT(s, quant_bytes);
                PUT(s, total_bytes);
                j.put_layout("layout", s.layout).put_slot(s.slot, {{"hist", s.slot_hist}, {"quantiles", s.slot_quant}});
            }
            j.end();
        }
        j.end();
    }
    j.emit();
    return 0;
}

// the spaces of a baseline that runs in several: "sp": [one put_trend object per space that is on, null for one that is off]
template <class PutSpace>
static void put_spaces(Json& j, u32 spaces, u32 n_spaces, ull slots, PutSpace put) {
    j.arr("sp");
    for (u32 k = 0; k < n_spaces; k++) {
        if (!((spaces >> k) & 1u)) { j.null(); continue; }
        j.obj().kv("slots", slots);
        put(k);
        j.end();
    }
    j.end();
}

// quantile_trend  "spaces on permille n_q q0 .. q7 ncap max_edges nc slots struct_size shift warmup ttl max_entries lat_floor_ns
// err_floor reserved": plan_quantile_trend's verdict, the tracked index and "sp" over [nodes, group edges, workloads]
static int stage_quantile_trend(const std::string& line) {
    Numbers n(line);
    const ull spaces = n(), on = n(), permille = n(), nq = n();
    u32 qm[8];
    for (u32& q : qm) q = (u32)n();
    const ull ncap = n(), me = n(), nc = n(), slots = n();
    const sg_trend_params p = read_trend_params(n);
    QuantTrendPlan P;
    const int rc = plan_quantile_trend(p, (u32)spaces, (u32)on, (u32)permille, qm, (u32)nq, (u32)ncap, me, (u32)nc, (u32)slots, &P);
    Json j;
    j.kv("rc", rc).kv("slots", slots).kv("ncap", ncap).kv("max_edges", me).kv("nc", nc).kv("node_trend_size", sizeof(sg_node_trend));
    j.kv("trend_size", sizeof(sg_edge_trend));
    if (rc == SG_OK) {
        PUT(P, spaces); PUT(P, qi); PUT(P, total_bytes);
        put_spaces(j, P.spaces, 3, slots, [&](u32 k) { put_trend(j, P.params[k], P.sp[k]); PUT(P.params[k], lat_floor_ns); PUT(P.params[k], err_floor); });
    }
    j.emit();
    return 0;
}

// traffic_trend  "spaces on max_edges ncap nc slots struct_size shift warmup ttl max_entries load_floor_ns rate_floor reserved":
// plan_traffic_trend's verdict, the resolved floors (as the struct names them and as the walk gets them) and "sp" over [edges,
// nodes, group edges, workloads]
static int stage_traffic_trend(const std::string& line) {
    Numbers n(line);
    const ull spaces = n(), on = n(), me = n(), ncap = n(), nc = n(), slots = n();
    sg_traffic_params p{};
    p.struct_size = (u32)n(); p.shift = (u32)n(); p.warmup = (u32)n(); p.ttl = (u32)n(); p.max_entries = n(); p.load_floor_ns = n();
    p.rate_floor = (u32)n(); p.reserved = (u32)n();
    TrafficPlan P;
    const int rc = plan_traffic_trend(p, (u32)spaces, (u32)on, me, (u32)ncap, (u32)nc, (u32)slots, &P);
    Json j;
    j.kv("rc", rc).kv("slots", slots).kv("ncap", ncap).kv("max_edges", me).kv("nc", nc).kv("node_trend_size", sizeof(sg_node_trend));
    j.kv("trend_size", sizeof(sg_edge_trend)).kv("params_size", sizeof(sg_traffic_params));
    if (rc == SG_OK) {
        PUT(P, spaces); PUT(P, rate_floor); PUT(P, load_floor_ns); PUT(P, lat_floor); PUT(P, err_floor); PUT(P, total_bytes);
        put_spaces(j, P.spaces, kTrafficSpaces, slots, [&](u32 k) { put_trend(j, P.params[k], P.sp[k]); });
    }
    j.emit();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------- main

static int print_option(const std::string& stage, const std::string& opt) {
    Json j;
    if (stage == "plan" && opt == "--knobs") { for (const KnobName& k : kKnobs) std::printf("%s\n", k.name); return 0; }
    if (stage == "plan" && opt == "--domains") {
        put_keys(j, "k1a_wide", kK1aWideKeys); put_keys(j, "k1a_tile", kK1aTileKeys); put_keys(j, "k1a_team", kK1aTeamKeys);
        put_keys(j, "k1b_merge", kK1bMergeKeys); put_keys(j, "k1b_stream", kK1bStreamKeys); put_keys(j, "k4_layer", kK4LayerKeys);
        j.kv("k1b_warm_u", kK1bWarmU);
    } else if (stage == "pair" && opt == "--domains") {
        put_keys(j, "k1a_team", kK1aTeamKeys); put_keys(j, "k1a_team_pair", kK1aTeamPairKeys);
    } else {
        std::fprintf(stderr, "%s takes no option %s\n", stage.c_str(), opt.c_str());
        return 2;
    }
    j.emit();
    return 0;
}

int main(int argc, char** argv) {
    static const struct { const char* name; int (*fn)(const std::string& line); } stages[] = {
        {"plan", stage_plan}, {"pair", stage_pair}, {"k5_form", stage_k5_form}, {"k5_efeat", stage_k5_efeat}, {"k3_forms", stage_k3_forms},
        {"prepare_fold", stage_prepare_fold}, {"select", stage_select}, {"trend", stage_trend}, {"vanish", stage_vanish}, {"nodes", stage_nodes},
        {"node_trend", stage_node_trend}, {"rank", stage_rank}, {"incident", stage_incident}, {"track", stage_track}, {"group", stage_group},
        {"group_trend", stage_group_trend}, {"group_nodes", stage_group_nodes}, {"group_rank", stage_group_rank},
        {"group_incident", stage_group_incident}, {"group_track", stage_group_track}, {"group_impact", stage_group_impact},
        {"quantile", stage_quantile}, {"quantile_trend", stage_quantile_trend}, {"traffic_trend", stage_traffic_trend},
    };
    const std::string stage = argc > 1 ? argv[1] : "";
    for (const auto& s : stages) {
        if (stage != s.name) continue;
        if (argc > 2) return print_option(stage, argv[2]);
        std::string line;
        while (std::getline(std::cin, line)) {
            if (line.empty() || line[0] == '#') continue;
            if (const int rc = s.fn(line)) return rc;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: plan_driver <stage> [--knobs | --domains]\nstages:");
    for (const auto& s : stages) std::fprintf(stderr, " %s", s.name);
    std::fprintf(stderr, "\n");
    return 2;
}
