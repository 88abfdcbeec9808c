// sg_plan.hpp — the engine's launch plan: every sizing decision sg_create and the launches take, computed from the config,
// two facts of the device and the development build's overrides.
//
// One place for the rules that each round retunes (which K1 path a window takes, partitions and pass-B table slots, the pass-A
// cache and its teams, warm-window state, the close's slices / splits / grids), each with the measured reason it has.
// It also chooses the kernel instantiation of every launch site that has several (Kernels) and lists the instantiations the
// library holds (k*Keys), which servicegraph.hip expands into its kernel tables.
// It owns the memory layout of every opt-in stage too: each plan_* cuts its stage's one device block with Block and keeps the
// offsets beside the sizes, so that servicegraph.hip only adds an offset to the block's base.
// No HIP in this file: tests/micro/plan_driver.cpp, stage plan, drives it on the CPU and tests/test_plan.py compares its plans with the
// ones the engine made before it existed (tests/golden/plans.json).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <optional>
#include <string>
#include <vector>

#include "../../include/servicegraph.h"
#include "sg_sizes.h"

namespace sgplan {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr size_t kLdsBytes = 160 * 1024;  // per workgroup on gfx950
constexpr int kStageSlots = 32;           // staging ring slots at most (Plan::n_stage of them are allocated)
constexpr size_t kPrepareLds = 4096;      // at least sizeof(KcScratch) (sg_k2.h; servicegraph.hip asserts it): what a folded close's prepare workgroup takes of pass B's dynamic LDS

inline u32 next_pow2(u64 v) { u64 p = 1; while (p < v) p <<= 1; return (u32)p; }
inline int grid_for(u64 items, int per_block, int cap = 2048) {
    u64 g = (items + per_block - 1) / per_block;
    return (int)std::max<u64>(1, std::min<u64>(g, (u64)cap));
}

struct DeviceFacts {
    int cus = 256;                        // compute units
    size_t lds_bytes = kLdsBytes;         // LDS per workgroup
};

// Tuning knobs (tools/k1_sweep.py, the A/B tests of alternative kernel paths): read from the environment by the DEVELOPMENT build
// only (-DSG_DEV_KNOBS -> lib/libservicegraph_dev.so); the shipped library plans with Overrides{}.  An override that is not a legal
// value is ignored by the rule it overrides.
struct Overrides {
    typedef std::optional<std::string> Knob;
    Knob ablate, np, ht, ct, nwg, nsub, split, warm, k1a, k1_narrow, k1_legacy, k1b_u, k1b_threads, k1b_pack, k1b_no_order,
         l2_global, l2_u32, dh_g, k3_slices, k3_no_fuse, k4_fused, k5_grid, k6_one_wg, dense_valu, copy_streams, stage_slots, arena, no_fold, k1a_pair, k5_form, k5_efeat, k3_in_form, k3_feat_lanes;
};
struct KnobName { const char* name; Overrides::Knob Overrides::*field; };
// the one list of knob names (alaz_amd/engine.py DEV_KNOBS is checked against it)
constexpr KnobName kKnobs[] = {
    {"SG_ABLATE", &Overrides::ablate}, {"SG_NP", &Overrides::np}, {"SG_HT", &Overrides::ht}, {"SG_CT", &Overrides::ct},
    {"SG_NWG", &Overrides::nwg}, {"SG_NSUB", &Overrides::nsub}, {"SG_SPLIT", &Overrides::split}, {"SG_WARM", &Overrides::warm},
    {"SG_K1A", &Overrides::k1a}, {"SG_K1_NARROW", &Overrides::k1_narrow}, {"SG_K1_LEGACY", &Overrides::k1_legacy},
    {"SG_K1B_U", &Overrides::k1b_u}, {"SG_K1B_THREADS", &Overrides::k1b_threads}, {"SG_K1B_PACK", &Overrides::k1b_pack},
    {"SG_K1B_NO_ORDER", &Overrides::k1b_no_order}, {"SG_L2_GLOBAL", &Overrides::l2_global}, {"SG_L2_U32", &Overrides::l2_u32},
    {"SG_DH_G", &Overrides::dh_g}, {"SG_K3_SLICES", &Overrides::k3_slices}, {"SG_K3_NO_FUSE", &Overrides::k3_no_fuse},
    {"SG_K4_FUSED", &Overrides::k4_fused}, {"SG_K5_GRID", &Overrides::k5_grid}, {"SG_K6_ONE_WG", &Overrides::k6_one_wg},
    {"SG_DENSE_VALU", &Overrides::dense_valu}, {"SG_COPY_STREAMS", &Overrides::copy_streams}, {"SG_STAGE_SLOTS", &Overrides::stage_slots},
    {"SG_ARENA", &Overrides::arena}, {"SG_NO_FOLD", &Overrides::no_fold}, {"SG_K1A_PAIR", &Overrides::k1a_pair},
    {"SG_K5_FORM", &Overrides::k5_form}, {"SG_K5_EFEAT", &Overrides::k5_efeat},
    {"SG_K3_IN_FORM", &Overrides::k3_in_form}, {"SG_K3_FEAT_LANES", &Overrides::k3_feat_lanes},
};
#ifdef SG_DEV_KNOBS
inline Overrides from_env() {
    Overrides o;
    for (const KnobName& k : kKnobs) if (const char* v = std::getenv(k.name)) o.*k.field = std::string(v);
    return o;
}
#endif
inline int ival(const Overrides::Knob& k) { return std::atoi(k->c_str()); }
inline u64 uval(const Overrides::Knob& k) { return std::strtoull(k->c_str(), nullptr, 0); }

struct Plan {
    // K1 (Dev fields of the same names)
    u32 variant = 0, narrow = 0, hist = 0, agg_slots = 3, nb = 0, np = 0, pb = 0, nwg = 256, k1b_split = 1, k1b_ht = 0, npb = 0, rb = 0,
        pcap = 0, sa = 0, sn = 0, sw = 0, punits = 0, ss = 0, pslots = 0, ovf_cap = 0, warm = 0;
    u32 k1b_threads = 1024, k1b_u = 4;
    bool k1b_pack = false;                    // narrow pass B: count + duration sum of a record in one 64-bit LDS add (sn x nwg < 2^16)
    bool k1b_order = false;                   // narrow pass B takes its partitions largest first (sg_k2.h kc_prepare)
    size_t k1b_lds = 0;                       // pass B's dynamic LDS (variant 0)
    bool prepare_fold = false;                // a close that tries the warm path launches no kc_prepare: its work rides in the warm attempt's launch (close_folds)
    // table sizes
    u32 ecap = 0, obcap = 0, ob_list_cap = 0, ncap = 0, max_obip = 1, alive_cap = 0, hub_cap = 0, max_blocks = 0;
    u64 kept_edges = 0;                       // arrays the rebuild indexes by KEPT position on a warm engine: max(max_edges, npb x pcap), else max_edges
    u32 max_known = 0;
    // the close
    u32 k3_ranges = 1, k3_slices = 8;
    size_t k3in_lds = 0;
    u32 k2_sortw = 0, dh_g = 0, dh_ppw = 0, dh_ns = 0;
    bool k4_split = false;                    // K4 in two launches per layer (gather, then the dense tiles)
    u32 k5_grid = 0;
    u32 k5_form = 0;                          // k5_edge_score: 0 = sixteen lanes per edge, 1 = one lane per edge (k5_edge_score_lanes); k5_grid is the form's own
    u32 k5_efeat = 0;                         // form 1 only: the score kernel computes the edge features itself — k3_node_features launches no edge workgroups, efeat / latz / errr do not exist
    u32 k3_in_form = 0;                       // k3_in_part: 0 = the loads of a trip under their tests, 1 = all of a trip's loads unconditional and issued together (k3_in_part<1>)
    u32 k3_feat_lanes = 0;                    // k5_efeat only (no edge workgroups): k3_node_features_lanes — eight lanes per node, the partials in one round trip
    bool k3_fuse_allowed = true;              // the one-call pipelines may fold k3_in_reduce into k3_in_part's launch
    bool k6_one_wg = false;                   // the round-3 single-workgroup halo-list builder
    bool use_mfma = true;
    // host resources
    u32 cus = 1;                              // compute units (pass B's "one round" arithmetic)
    int k1_grid = 0, n_copy = 1, n_stage = 16;
    bool arena_on = false;
    u32 n_slots = 1;                          // window slots in flight
    u32 ablate = 0;
};

// pass A's geometry: follows the join tables' state (the engine re-plans it whenever they change)
struct PassA {
    bool l2_u16 = false, k1a_team = false, l2_in_lds = false;
    u32 k1a_nsub = 2, k1a_teams = 2, k1a_nt = 1024, k1a_ct = 2048;
    size_t k1a_lds = 0;
    // the team kernel's paired form (sg_k1_team.h PAIR): a team copies two tiles out together.  k1a_lds stays the sum of the layout both
    // forms share; k1a_pair_lds is what the paired form's second tile per team takes on top (0 without): a launch asks for both
    bool k1a_pair = false;
    size_t k1a_pair_lds = 0;
};

// struct_size / ABI / range checks and the config's defaults (0 = max_batch / max_known_nodes / max_batch)
inline int check_config(const sg_config& in, sg_config* out) {
    // ABI 3: the caller states how much of sg_config it knows about; the rest is zero
    constexpr uint32_t kCfgMin = 88;                                 // sizeof(sg_config) when struct_size was introduced
    if (in.struct_size < kCfgMin || in.struct_size > 4096) return SG_EINVAL;
    sg_config c; std::memset(&c, 0, sizeof c);
    std::memcpy(&c, &in, std::min<size_t>(in.struct_size, sizeof c));
    c.struct_size = (uint32_t)sizeof c;
    if (c.abi_version != SG_ABI_VERSION || c.layers < 1 || c.layers > SG_MAX_LAYERS || c.max_edges == 0 ||
        c.max_known_nodes == 0 || c.world == 0 || c.rank >= c.world || c.max_known_nodes > 0x3FFFFFFFu)
        return SG_EINVAL;
    if (c.max_batch == 0) c.max_batch = 1u << 20;
    if (c.max_ips == 0) c.max_ips = c.max_known_nodes;
    if (c.max_window_events == 0) c.max_window_events = c.max_batch;
    *out = c;
    return SG_OK;
}

// cfg: as check_config left it
// k5_edge_score's form (sg_k5.h).  Where nobody asks by name the plan takes form 1 where it was measured to win — unsharded engines of
// a million edges and more, the C3 shape (same-box A/B: profiles/k5_lanes_ab_c3.txt) — and form 0 everywhere else: C2 and the C5
// shards are not measured yet.  Form 1's footprint: LDS per workgroup (4 waves x K5L_WAVE_LDS) and the waves per SIMD its registers
// allow (amdgpu_waves_per_eu).
constexpr u64 kK5LanesMinEdges = 1ull << 20;
inline u32 k5_form_default(const sg_config& cfg) { return cfg.world <= 1 && cfg.max_edges >= kK5LanesMinEdges ? 1u : 0u; }
// Form 1 with the edge features inline (k5_edge_score_lanes<.., true>): what an engine of form 1 takes unasked, set by the same-box A/B
// of profiles/k5_efeat_ab_c3.txt; SG_K5_EFEAT=0/1 names it in the development build.  It exists for form 1 only.
constexpr bool kK5EfeatDefault = true;
// K3's batched loads, each behind its own constant, set by the same-box A/B of profiles/k3_forms_ab_c3.txt.  k3_in_part<1>: lower in every
// round there, so an engine of the measured shape takes it unasked — the shape of K5's form 1 (C3); C2 and a config-5 shard were not
// measured and keep form 0.  k3_node_features_lanes (node-only launches, k5_efeat): its kernel is shorter but the window was not lower in
// every round, so it stays behind SG_K3_FEAT_LANES=1 in the development build.
constexpr bool kK3InFormDefault = true, kK3FeatLanesDefault = false;
inline u32 k3_in_form_default(const sg_config& cfg) { return kK3InFormDefault && k5_form_default(cfg) ? 1u : 0u; }
constexpr size_t kK5LanesWgLds = 4 * 8192;
constexpr int kK5LanesWaves = 3;
constexpr int k5_lanes_wgs_per_cu() { return (int)std::min<size_t>(kLdsBytes / kK5LanesWgLds, (size_t)kK5LanesWaves); }
inline int make_plan(const sg_config& cfg, const DeviceFacts& dev, const Overrides& ov, Plan* out, std::string* why) {
    sg_config chk;
    if (check_config(cfg, &chk) != SG_OK) { if (why) *why = "invalid config"; return SG_EINVAL; }
    Plan p;
    const size_t lds = dev.lds_bytes;
    // SG_ARENA=1: everything below 32 MiB is carved out of 256 MiB chunks instead of one hipMalloc per array (a test of whether the
    // small arrays' page-table entries cost the window close — a chain of small latency-bound kernels — anything: measured on one box,
    // 507.7 / 508.3 us per C3 window with the chunks, 505.1 / 504.8 without; off).
    if (ov.arena) p.arena_on = ival(ov.arena) != 0;
    p.k1_grid = std::min<int>(SG_MAX_K1_WGS, dev.cus * 8);
    p.cus = (u32)std::max(1, dev.cus);
    p.use_mfma = !(ov.dense_valu && (*ov.dense_valu)[0] == '1');
    p.max_known = cfg.max_known_nodes;

    const u64 ME = cfg.max_edges;
    p.ecap = next_pow2(std::max<u64>(2 * ME, K2_TILE));
    p.obcap = next_pow2(std::max<u64>(2 * (u64)cfg.max_outbound_ips, 64));
    p.ob_list_cap = next_pow2(std::max<u64>((u64)cfg.max_outbound_ips * std::max<u32>(cfg.world, 1), 64));
    p.max_obip = std::max<u32>(cfg.max_outbound_ips, 1);
    p.ncap = cfg.max_known_nodes + cfg.max_labels + p.max_obip;

    // K1 variant: 0 = partitioned LDS aggregation (fast; bounded edges per partition), 1 = global table + atomics
    p.variant = cfg.k1_variant == 1 ? 1u : 0u;
    p.hist = (cfg.flags & SG_CFG_EDGE_HISTOGRAM) ? 1u : 0u;
    p.agg_slots = p.hist ? 5u : 3u;
    // Narrow-record K1 (default): an endpoint is a compact index below 2^nb — KNOWN ids, then LABEL ids, then slots of the
    // outbound-IP table — and the mixed pair's top bits are the partition (sg_hash.h sg_kmix); it needs the in-partition
    // remainder of the key to fit 31 bits.  k1_variant 2 (or SG_K1_LEGACY) keeps the 16-byte-record kernels, which also
    // carry the per-edge histogram.
    const u64 cn = (u64)cfg.max_known_nodes + cfg.max_labels + p.obcap;
    u32 nb = 12; while ((1ull << nb) < cn && nb < 31) nb++;
    bool narrow = p.variant == 0 && !p.hist && cfg.k1_variant != 2 && !ov.k1_legacy && nb <= 24;
    // k1_variant 0 (auto) picks by the WINDOW, not only by what fits: the 8-byte path pays from a few million events or a quarter
    // of a million edges per window up; below that (BASELINE config 2: 1 M events, 54 k edges) a window is a dozen launches of
    // 5-30 us and the 16-byte kernels' shorter prologue and simpler pass B win — same box, C2: 130 us per window against 147-155
    // (three rounds of tuning for config 3 had been paid for at config 2).  3 asks for the 8-byte path by name.
    const bool small_window = ME < (1ull << 18) && cfg.max_window_events <= (2ull << 20);
    if (cfg.k1_variant == 0 && small_window && !ov.k1_narrow) narrow = false;
    u64 np = 0;
    if (narrow) {
        // partitions: ~2700 distinct edges each at the configured capacity at most (pass B's LDS table: 4096 slots of 36
        // bytes, 3072 may fill), at least 256.  Fewer partitions = longer runs per tile in pass A.
        np = next_pow2(std::max<u64>((ME + 2699) / 2700, 256));
        u32 pbt = 0; while ((1ull << pbt) < np) pbt++;
        if (np > 2048 || 2 * nb - pbt > 31) narrow = false;          // (one wave scans the run lengths: beyond this the 16-byte kernels / variant 1)
    }
    p.k1b_split = 1;
    if (narrow) {
        // pass B: a partition that may hold more than ~1150 edges is merged by TWO workgroups (sub-tables of 2048 slots, two
        // workgroups per CU) rather than by one with a 4096-slot table that owns the CU alone
        if (ME / np > 1150) { p.k1b_split = 2; p.k1b_ht = 2048; }
        else p.k1b_ht = ME / np > 550 ? 2048 : 1024;
        // (sizing the partitions by the window's RECORDS as well — 512 x 2 workgroups for a shard of C4, 10 M events over 126 k
        // edges — was measured and bought nothing: 79 vs 73 us)
        if (ov.split) { const int x = ival(ov.split); if (x == 1 || x == 2) { p.k1b_split = (u32)x; p.k1b_ht = ME / (np * x) > 1150 ? 4096 : (ME / (np * x) > 550 ? 2048 : 1024); } }
    } else {
        // 16-byte records: at most ~1250 distinct edges per partition (pass B's LDS table: 2048 slots, 1536 may fill; 1024 slots
        // for small graphs), at least one per CU.  C3 with 1024 partitions 181 us, 2048: 198 us, 4096: 292 us.
        np = next_pow2(std::max<u64>((ME + 1249) / 1250, 256));
        if (np > 4096) np = 4096;
        if (cfg.k1_variant != 1 && ME > (u64)4096 * 1400) p.variant = 1;   // beyond the partitioned path's range
        p.k1b_ht = ME / np > 600 ? 2048 : 1024;
        if (p.hist && p.k1b_ht == 2048) { p.k1b_ht = 1024; np = std::min<u64>(4096, np * 2); }   // 16 x u32 bins per slot: 104 bytes, half the slots, twice the partitions
    }
    p.np = (u32)np; p.nwg = 256;
    // tuning overrides (tools/k1_sweep.py); anything that is not a legal geometry is ignored
    if (ov.np) { const u64 x = uval(ov.np); if (x >= 64 && x <= (narrow ? 2048u : 4096u) && (x & (x - 1)) == 0) p.np = (u32)x; }
    if (ov.ht) { const u64 x = uval(ov.ht); if (x >= 256 && x <= (narrow ? 4096u : 2048u) && (x & (x - 1)) == 0) p.k1b_ht = (u32)x; }
    if (ov.nwg) { const u64 x = uval(ov.nwg); if (x >= 1 && x <= (u64)SG_MAX_K1_WGS) p.nwg = (u32)x; }
    p.pb = 0; while ((1u << p.pb) < p.np) p.pb++;
    if (narrow && 2 * nb - p.pb > 31) { p.np = (u32)np; p.pb = 0; while ((1u << p.pb) < p.np) p.pb++; }   // an SG_NP override that would not leave 31 remainder bits
    p.narrow = (narrow && p.variant == 0) ? 1u : 0u;
    if (!p.narrow) p.k1b_split = 1;
    // warm windows: the 8-byte-record path without the per-edge histogram (whose bins would have to follow the kept order too);
    // SG_CFG_NO_WARM / SG_WARM=0 keep every window on the full rebuild.  (k1b_u = 8, the one-table-per-CU build, has no warm instantiation.)
    // By default only where it pays: on a graph below a quarter of a million edges the rebuild's four kernels cost about what the
    // compaction plus their four empty launches do (C2, same box: 147 us per window without, 155 with).  SG_CFG_WARM asks for it anyway.
    p.warm = (p.narrow && !p.hist && !(cfg.flags & SG_CFG_NO_WARM) && ((cfg.flags & SG_CFG_WARM) || ME >= (1ull << 18))) ? 1u : 0u;
    if (ov.warm) p.warm = (ival(ov.warm) != 0 && p.narrow && !p.hist) ? 1u : 0u;
    p.npb = p.np * p.k1b_split;
    p.nb = nb; p.rb = 2 * nb - p.pb;
    p.pcap = p.narrow ? p.k1b_ht * 13 / 16 : p.k1b_ht * 3 / 4;       // (u32 keys probe cheaply: the narrow tables may fill to 0.81)
    const double m = (double)cfg.max_window_events / ((double)p.np * p.nwg);
    p.sa = std::min<u32>(24, std::max<u32>(8, (2 * 2048 / p.np + 6 + 1) & ~1u));   // aggregates per piece: cache slots / partitions, with head room
    if (p.narrow) {
        // a hot key the cache missed lands in ONE piece: twice the mean + 8 sigma + 24 records, then the overflow list
        p.sn = ((u32)(2.0 * m + 8.0 * std::sqrt(m + 1.0) + 24.0) + 1u) & ~1u;
        p.sn = std::min<u32>(p.sn, (1u << 20) - 16);
        p.sw = std::min<u32>(64, std::max<u32>(8, p.sn / 8));
        p.punits = (p.sn + 2 * p.sw + 5 * p.sa + 15) / 16 * 16;     // a piece = whole 128-byte lines; the slack goes to the narrow region
        p.sn = p.punits - 2 * p.sw - 5 * p.sa;
        p.ss = 0; p.pslots = 0;
    } else {
        p.ss = (u32)(2.0 * m + 8.0 * std::sqrt(m + 1.0) + 24.0);          // a hot key the cache missed lands in ONE piece: head room, then the overflow list
        p.ss = (p.ss + p.agg_slots * p.sa + 7) / 8 * 8 - p.agg_slots * p.sa;   // a piece = whole 128-byte lines
        p.ss = std::min<u32>(p.ss, (1u << 20) - 8);
        p.pslots = p.ss + p.agg_slots * p.sa;
    }
    p.ovf_cap = 1u << 16;
    p.k1b_threads = 1024u;                                          // measured: 1024 threads beat 2 x 512 (C3 135 vs 153 us, C2 15.5 vs 22.9 us)
    // pass B's LDS table (narrow: accumulators, keys, two counters, then the warm path's touch bits and new-key bits — one each per slot
    // — and three words; 16-byte records: key, accumulators and the histogram's bins per slot)
    if (p.variant == 0)
        p.k1b_lds = p.narrow ? ((size_t)p.k1b_ht * 36 + 8 + (size_t)p.k1b_ht / 4 + 12 + 15) / 16 * 16 : (size_t)p.k1b_ht * (8 + 32 + (p.hist ? 4 * SG_HIST_BINS : 0));
    // narrow pass B: 8 x 16 bytes per lane in flight where a CU holds one table anyway; two workgroups per CU need <= 64 VGPRs
    if (p.narrow) p.k1b_u = 2 * p.k1b_lds > lds && m > 24.0 ? 8 : 4;
    if (ov.k1b_u) { if (ival(ov.k1b_u) == 8) p.k1b_u = 8; if (ival(ov.k1b_u) == 4) p.k1b_u = 4; }
    if (p.k1b_u == 8) p.warm = 0;
    // the packed add of pass B is exact while a workgroup merges fewer than 2^16 narrow records: a partition's pieces hold sn each
    p.k1b_pack = p.narrow && (u64)p.sn * p.nwg < 65536ull;
    if (ov.k1b_pack) { if (ival(ov.k1b_pack) == 0) p.k1b_pack = false; }
    if (ov.k1b_threads) { const u64 x = uval(ov.k1b_threads); if ((x == 256 && !p.narrow) || x == 512 || x == 1024) p.k1b_threads = (u32)x; }
    if (p.narrow && p.k1b_ht / p.k1b_threads > 4) p.k1b_threads = 1024u;    // (the compaction takes at most four table slots per thread)
    p.k1b_order = p.narrow && !ov.k1b_no_order;
    // Warm closes without the kc_prepare launch (sg_k2.h kc_prepare_rest): one 1 024-thread workgroup, ~7 us of dependent round trips between
    // pass A and pass B while the rest of the chip waits.  Where the close launches the warm attempt, that workgroup's work becomes one MORE
    // workgroup of the attempt's launch (it runs beside the merge), every merge workgroup takes the warm / cold decision itself, and the order
    // of the partitions is one window older (two buffers by window parity).  Only the shape that was built for: a variant-0 narrow engine that
    // keeps state, unsharded, whose pass B runs 1 024 threads (the prepare workgroup's strides) over an LDS that holds kc_prepare's scratch.
    // SG_NO_FOLD=1 keeps the separate launch (the A/B twin of tests/test_gpu_prepare_fold.py).
    p.prepare_fold = p.warm && p.narrow && p.variant == 0 && cfg.world <= 1 && p.k1b_threads == 1024u && p.k1b_lds >= kPrepareLds &&
                     !(ov.no_fold && ival(ov.no_fold) != 0);
    // join tables: IP blocks of the two-level table (variant 1 probes the cuckoo table only)
    p.max_blocks = p.variant == 0 ? (u32)std::min<u64>(1024, std::max<u64>(64, (u64)cfg.max_ips / 32)) : 2u;
    if (p.variant == 0) p.ecap = K2_TILE;                            // the global edge table is not used
    p.alive_cap = cfg.max_alive ? cfg.max_alive : 65536u;
    p.kept_edges = p.warm ? std::max<u64>(ME, (u64)p.npb * p.pcap) : ME;
    p.hub_cap = (u32)std::min<u64>(p.kept_edges / 256 + 16, 1u << 24);   // blocks of the rows longer than one block: at most E / 512 + one per such row

    p.k3_ranges = (p.ncap + K3_IN_NR - 1) / K3_IN_NR;
    // slices of the in-statistics' scan: 8 192 edges each at least; at most 48 where ranges x 48 workgroups (one per CU: 144 KiB of LDS) are ONE
    // round of the chip — since the node features sum the partials themselves (k3_in_reduce is gone from the one-call pipelines) the shorter scan
    // wins: same box, C3, K3-in + K3-feat 53.5-54.4 us at 32 slices, 49.6-49.8 at 48, 53.4 at 51 (profiles/r06_k3slices_ab_c3.txt) — else 32 (a
    // config-5 shard's 49 ranges: more slices only add partials to write and read)
    p.k3_slices = (u32)std::min<u64>((u64)p.k3_ranges * K3_IN_SMAX <= p.cus ? K3_IN_SMAX : 32, std::max<u64>(8, ME / 8192));
    if (ov.k3_slices) { const u64 x = uval(ov.k3_slices); if (x >= 1 && x <= 256) p.k3_slices = (u32)x; }
    p.k3in_lds = (size_t)K3_IN_NR * 48;
    {   // the row sort's two LDS arrays: large enough for a bitmap of the node capacity when that fits (a config-5 shard: 150 k nodes = 4.7 k words)
        const u64 bw = ((u64)p.ncap + 31) / 32;
        p.k2_sortw = bw <= K2_SORT_LDS ? K2_SORT_LDS : (u32)std::min<u64>(K2_SORT_LDS_MAX, (bw + 255) / 256 * 256);
    }
    {   // row degrees / in-row ranks by LDS histograms instead of one returning device atomic per edge (k2_deg_hist): when a u32 counter
        // per node fits one workgroup's LDS.  G workgroups of npb / G consecutive output partitions each (G a power of two, 16 .. K2_DH_GMAX).
        u32 g = std::min<u32>(K2_DH_GMAX, p.variant == 0 ? p.npb : 0u);            // (k2_rowptr: a multiple of 16)
        // small graphs keep the degree atomics: their cost grows with the edges (1 M: 23 us of pass B), the histogram launch and the wider
        // row scan cost 6-7 us whatever the size — C2 (66 k-edge capacity), same box: window 128.5 / 130.2 us with it, 124.4 / 125.3 without
        if (ME < (1ull << 19)) g = 0;
        // an engine that keeps warm-window state rebuilds rarely, and every launch of the rebuild chain is ~4.5 us of an EMPTY launch on a
        // warm window: there the degree atomics (23-30 us more on a cold window at C3, no launch) are the better trade.  (SG_DH_G cannot
        // switch the histogram on for such an engine: its delta windows rank the new edges with the degree replicas.)
        if (p.warm) g = 0;
        else if (ov.dh_g) { const u64 x = uval(ov.dh_g); g = (x >= 16 && x <= K2_DH_GMAX && (x & (x - 1)) == 0 && p.variant == 0 && x <= p.npb) ? (u32)x : 0u; }
        if (g >= 16 && (g & (g - 1)) == 0 && p.npb % g == 0 && ((size_t)p.ncap + 1) * sizeof(u32) <= 128u * 1024u && (u64)p.npb * p.pcap < (1ull << 32)) {
            p.dh_g = g; p.dh_ppw = p.npb / g; p.dh_ns = (p.ncap + 1 + 63u) & ~63u;
        }
    }
    p.ablate = ov.ablate ? (u32)std::strtoul(ov.ablate->c_str(), nullptr, 0) : 0u;
    // K4: two launches per layer — the gather-mean at high occupancy (8 rows per workgroup), then the dense tiles.  Small graphs keep
    // the fused kernel: at C2 the second launch costs more than the gather gains — 16.6 vs 20.9 us.  (C2's 66 k-edge engine stays fused;
    // a 160 k-edge shard of C4 — with its hub rows — splits.)
    p.k4_split = cfg.max_edges > (1u << 17);
    if (ov.k4_fused) p.k4_split = ival(ov.k4_fused) == 0;
    // K5: ONE round of workgroups: the kernel runs 3 waves per SIMD (144 registers, amdgpu_waves_per_eu(3)) = 3 workgroups of 256 threads per CU at a
    // time, and its waves stride over the edges — 2 048 workgroups were 2.67 rounds, the last one two-thirds empty.  Same box, C3, two
    // repetitions: K5 61.1 us at 2 048, 61.7 at 1 024, 58.9 at 1 536, 57.8-57.9 at 768 (profiles/r06_grids_ab_c3.txt)
    p.k5_form = k5_form_default(cfg);
    if (ov.k5_form) {                                                // (an unknown form is refused, not ignored: an A/B that silently ran one form twice would look like a tie)
        if (*ov.k5_form != "0" && *ov.k5_form != "1") { if (why) *why = "SG_K5_FORM: 0 (sixteen lanes per edge) or 1 (one lane per edge)"; return SG_EINVAL; }
        p.k5_form = (u32)ival(ov.k5_form);
    }
    if ((u64)p.ncap * 256u > (1ull << 32)) p.k5_form = 0;            // form 1 addresses a P / Q row by a 32-bit byte offset
    // the features inline: the default follows the form; refused by name with form 0, which has no such kernel
    p.k5_efeat = p.k5_form && kK5EfeatDefault ? 1u : 0u;
    if (ov.k5_efeat) {
        if (*ov.k5_efeat != "0" && *ov.k5_efeat != "1") { if (why) *why = "SG_K5_EFEAT: 0 (k3_node_features stores the edge features) or 1 (k5_edge_score_lanes computes them)"; return SG_EINVAL; }
        p.k5_efeat = (u32)ival(ov.k5_efeat);
        if (p.k5_efeat && !p.k5_form) { if (why) *why = "SG_K5_EFEAT=1 needs form 1 of k5_edge_score (SG_K5_FORM)"; return SG_EINVAL; }
    }
    // form 0: 32 edges per workgroup and step, 3 workgroups per CU.  Form 1: 256 edges per workgroup and step; a CU holds
    // min(LDS / kK5LanesWgLds, kK5LanesWaves) of its workgroups (4 waves each, one per SIMD): one round of those
    const int k5_per_wg = p.k5_form ? 256 : 32, k5_round = (p.k5_form ? k5_lanes_wgs_per_cu() : 3) * (int)p.cus;
    p.k5_grid = (u32)grid_for(cfg.max_edges, k5_per_wg, k5_round);
    if (ov.k5_grid) { const int x = ival(ov.k5_grid); if (x >= 1 && x <= 65535) p.k5_grid = (u32)std::min(grid_for(cfg.max_edges, k5_per_wg, 65535), x); }
    // K3's two batched-load forms: each behind its own default, set by the same-box A/B of profiles/k3_forms_ab_c3.txt
    p.k3_in_form = k3_in_form_default(cfg);
    if (ov.k3_in_form) {
        if (*ov.k3_in_form != "0" && *ov.k3_in_form != "1") { if (why) *why = "SG_K3_IN_FORM: 0 (a trip's loads under their tests) or 1 (issued together)"; return SG_EINVAL; }
        p.k3_in_form = (u32)ival(ov.k3_in_form);
    }
    p.k3_feat_lanes = p.k5_efeat && kK3FeatLanesDefault ? 1u : 0u;
    if (ov.k3_feat_lanes) {
        if (*ov.k3_feat_lanes != "0" && *ov.k3_feat_lanes != "1") { if (why) *why = "SG_K3_FEAT_LANES: 0 (k3_node_features, two lanes per node) or 1 (k3_node_features_lanes, eight)"; return SG_EINVAL; }
        p.k3_feat_lanes = (u32)ival(ov.k3_feat_lanes);
        if (p.k3_feat_lanes && !p.k5_efeat) { if (why) *why = "SG_K3_FEAT_LANES=1 needs the edge features in the score kernel (SG_K5_EFEAT): the eight-lane kernel has no edge workgroups"; return SG_EINVAL; }
    }
    p.k3_fuse_allowed = !ov.k3_no_fuse;                              // (development build: the two-launch form beside the fused one on one box)
    p.k6_one_wg = (bool)ov.k6_one_wg;
    if (ov.copy_streams) p.n_copy = ival(ov.copy_streams) == 2 ? 2 : 1;
    if (ov.stage_slots) p.n_stage = std::min(kStageSlots, std::max(2, ival(ov.stage_slots)));
    p.n_slots = std::min<u32>(std::max<u32>(cfg.windows_in_flight, 1), 8);
    *out = p;
    return SG_OK;
}

// Pass A's geometry for join tables of l1_entries level-1 entries and l2_bytes of level-2 blocks: does level 2 fit LDS beside the
// edge cache (and, narrow path, the tile)?  Returns false when no legal geometry exists (the engine fails the call with a message
// instead of launching a kernel that asks for more than a CU's LDS).
// Does the plan take the team kernel's paired form where it fits?  Set by the same-box A/B of profiles/pair_tiles_ab_c3.txt.
constexpr bool kK1aPairDefault = true;
inline bool plan_pass_a(const Plan& p, uint32_t l1_entries, size_t l2_bytes, const Overrides& ov, PassA* out) {
    PassA a;
    const size_t lds_cap = kLdsBytes;
    const size_t l1b = (size_t)l1_entries * 8, l2b = l2_bytes;
    const size_t stage_max = (size_t)K1A_NJ * K1A_THREADS * 16;    // what the prologue can stage: six 16-byte words per lane
    if (p.narrow) {
        // cache | 6 counters per partition | statistics | tile | join tables.  Level 2 is staged as u16 entries
        // (half the bytes) when every node id fits 14 bits.
        a.l2_u16 = p.max_known <= 16384 && !ov.l2_u32;
        const size_t l2lds = a.l2_u16 ? l2b / 2 : l2b;
        if (ov.nsub) { const int x = ival(ov.nsub); if (x == 1 || x == 2) a.k1a_nsub = (u32)x; }
        // round 4: two teams per workgroup (k1a_team_partition) when their two tiles and counter sets fit beside a cache of 256 slots or
        // more; SG_K1A=tile keeps the one-team kernel (k1a_tile_partition), SG_K1A=team takes the two-team kernel whenever it fits at all
        const bool want_tile = ov.k1a && *ov.k1a == "tile", force_team = ov.k1a && *ov.k1a == "team";
        const size_t fixed_tile = (size_t)p.np * 24 + 64 + (size_t)K1T_TS(a.k1a_nsub) * 8 + l1b;
        // the two-team kernel is instantiated for 256 / 512 / 1024 partitions, 1024 threads (two teams of eight waves, one group of four events
        // per thread and tile: round 6; round 4 ran two groups at 768 threads) and a join blob its prologue can stage; everything else keeps
        // the one-team kernel
        const int teams = 2, nt = 1024;
        // (what the team kernel's prologue can stage: six 16-byte words per lane of its threads.  Level 1 always goes through it, level 2
        // only when it is staged — an engine whose level 2 stays in global memory needs room for level 1 alone)
        const size_t stage_team = (size_t)K1A_NJ * nt * 16;
        // (endpoint spaces beyond 15 bits — a shard of BASELINE config 5: 18 — leave no room for the partition number in a parked record: the
        // kernel's 16-lanes-per-run copy-out takes over, the workgroup has the 1024 threads it is written for since round 6)
        const bool team_ok = (p.np == 256 || p.np == 512 || p.np == 1024) && (size_t)p.np * p.nwg * p.punits * 8 < ((size_t)1 << 31) && l1b <= stage_team;
        a.k1a_teams = (u32)teams; a.k1a_nt = (u32)nt;
        const size_t fixed_team = K1M_LDS_FIXED(p.np, teams, nt) + l1b;
        auto pick = [&](size_t fixed, u32 ct_min, size_t stage_cap, u32& ct, bool& in_lds) {
            ct = 0; in_lds = false;
            // (the cache flattens the hottest keys; beyond 1024 slots it costs more aggregates than it saves records)
            for (u32 c : {1024u, 512u, 256u, 128u}) if (c >= ct_min && (size_t)c * 40 + fixed + l2lds <= lds_cap && l1b + l2b <= stage_cap) { in_lds = true; ct = c; break; }
            if (!ct) for (u32 c : {1024u, 512u, 256u, 128u, 64u}) if (c >= ct_min && (size_t)c * 40 + fixed <= lds_cap) { ct = c; break; }
        };
        u32 ct = 0; bool in_lds = false;
        if (!want_tile && team_ok) { pick(fixed_team, force_team ? 64u : 256u, stage_team, ct, in_lds); a.k1a_team = ct != 0; }
        if (!ct) pick(fixed_tile, 64u, stage_max, ct, in_lds);
        const size_t fixed = a.k1a_team ? fixed_team : fixed_tile;
        a.l2_in_lds = in_lds;
        if (ov.l2_global) a.l2_in_lds = false;
        if (ov.ct) { const u32 x = (u32)std::strtoul(ov.ct->c_str(), nullptr, 0); if (x >= 64 && x <= 2048 && (x & (x - 1)) == 0 && (size_t)x * 40 + fixed + (a.l2_in_lds ? l2lds : 0) <= lds_cap) ct = x; }
        if (!ct || l1b > stage_max) return false;
        a.k1a_ct = ct;
        a.k1a_lds = (size_t)ct * 40 + fixed + (a.l2_in_lds ? l2lds : 0);
        // the paired form: only BESIDE what was chosen above — the same cache, the same level-2 placement —, where a parked record carries
        // its partition number (2 nb <= 31: the move of a pair's first tile reads it there), for the partition counts it is instantiated
        // for, and by default only beside a cache of 512 slots or more.  The default never trades the cache for the second tile: a cache
        // the join tables have pushed below 512 slots leaves no 32 KiB anyway, and the one trade there is to make — 1 024 slots for 512 —
        // was measured at 1 024 partitions only (profiles/pair_tiles_ab_c3.txt).  SG_K1A_PAIR=1 takes pairs wherever they fit, with that
        // trade where it makes them fit (no SG_CT beside it); =0 takes them nowhere.
        {
            const size_t extra = K1M_LDS_PAIR_EXTRA(p.np, teams, nt);
            const bool able = a.k1a_team && 2 * p.nb <= 31 && (p.np == 256 || p.np == 512 || p.np == 1024);
            const bool forced = ov.k1a_pair && ival(ov.k1a_pair) != 0;
            if (able && forced && !ov.ct && ct > 512 && a.k1a_lds + extra > lds_cap && a.k1a_lds - (size_t)(ct - 512) * 40 + extra <= lds_cap) {
                a.k1a_lds -= (size_t)(ct - 512) * 40; ct = 512; a.k1a_ct = ct;
            }
            const bool fits = able && a.k1a_lds + extra <= lds_cap;
            // (1 024 partitions by name only: pairs were measured there as records arriving split, and lost)
            const bool want = ov.k1a_pair ? forced : (kK1aPairDefault && ct >= 512 && p.np <= 512);
            a.k1a_pair = fits && want;
            a.k1a_pair_lds = a.k1a_pair ? extra : 0;
        }
        *out = a;
        return true;
    }
    const size_t fixed = (size_t)p.np * 4 + 64 + l1b;
    const size_t slot = p.hist ? 72 : 40;                    // cache slot: key + 4 accumulators (+ 16 x u16 bins)
    u32 ct = 0;
    for (u32 c : {2048u, 1024u, 512u}) if ((size_t)c * slot + fixed + l2b <= lds_cap && l1b + l2b <= stage_max) { a.l2_in_lds = true; ct = c; break; }
    // level 2 stays in global memory: the largest cache that fits beside the counters and level 1
    if (!ct) for (u32 c : {2048u, 1024u, 512u, 256u, 128u, 64u}) if ((size_t)c * slot + fixed <= lds_cap) { ct = c; break; }
    if (ov.ct) { const u32 x = (u32)std::strtoul(ov.ct->c_str(), nullptr, 0); if (x >= 64 && x <= 2048 && (x & (x - 1)) == 0 && (size_t)x * slot + fixed + (a.l2_in_lds ? l2b : 0) <= lds_cap) ct = x; }
    if (ov.l2_global) a.l2_in_lds = false;
    if (!ct || l1b > stage_max) return false;
    a.k1a_ct = ct;
    a.k1a_lds = (size_t)ct * slot + fixed + (a.l2_in_lds ? l2b : 0);
    *out = a;
    return true;
}

// ---- which kernel instantiation each launch site runs -------------------------------------------------------------------------
// The template arguments of the kernel families that come in several instantiations, chosen from the plan: servicegraph.hip
// resolves them to kernel pointers through one table per family (at create, and pass A's again whenever it is re-planned), and
// tests/test_plan.py checks the choice on the CPU.  A field the chosen family does not take is 0.
enum K1aFamily { K1A_GLOBAL = 0, K1A_WIDE = 1, K1A_TILE = 2, K1A_TEAM = 3 };   // k1_resolve_aggregate, k1a_partition, k1a_tile_partition, k1a_team_partition
enum K1bFamily { K1B_NONE = 0, K1B_MERGE = 1, K1B_STREAM = 2 };                // (variant 1 has no pass B), k1b_merge, k1b_stream_merge
constexpr int kK1bWarmU = 2;                  // K1B_WARM_U (sg_k1_narrow.h): pass B's U on an engine that keeps warm state
struct PassAKernel {
    int family = K1A_GLOBAL;
    int l2 = 0;                               // level 2 of the join tables: 0 = global memory, 1 = LDS, 2 = LDS as u16 entries (tile, team)
    bool sharded = false, hist = false;       // (hist: k1a_partition only)
    int nsub = 0, pb = 0;                     // tile: sub-tiles (1, 2); team: log2 of the partitions (8, 9, 10)
    bool pair = false;                        // team: the paired form (kK1aTeamPairKeys)
};
struct Kernels {
    PassAKernel k1a;
    // pass B.  share: the SGPR-capped build (two workgroups share a CU) rather than its _wide twin.  warm: the engine launches the
    // warm attempt and the cold merge (WM 1 and 2, U = kK1bWarmU); a window it closes the plain way takes the WM 0 form with k1b_u.
    int k1b_family = K1B_NONE, k1b_u = 0, k1b_spt = 0;
    bool k1b_pack = false, k1b_hist = false, k1b_share = false, k1b_warm = false;
    bool k2_dh = false;                       // k2_rowptr over the degree histograms
    bool k4_split = false, k4_mfma = true;    // k4_sage_layer (input width, projection and threads follow the layer at launch)
    bool k5_mfma = true;                      // k5_node_proj (k5_edge_score's fused reset is the caller's argument)
    int k5_form = 0;                          // k5_edge_score (0) or k5_edge_score_lanes (1)
    int k5_efeat = 0;                         // k5_edge_score_lanes<.., EFEAT>: the edge features computed inline
    int k3_in_form = 0, k3_feat_lanes = 0;    // k3_in_part<FORM>; k3_node_features (0) or k3_node_features_lanes (1)
};
inline PassAKernel choose_pass_a(const Plan& p, const PassA& a, const sg_config& cfg) {
    PassAKernel k;
    if (p.variant != 0) return k;
    k.sharded = cfg.world > 1;
    if (!p.narrow) { k.family = K1A_WIDE; k.l2 = a.l2_in_lds ? 1 : 0; k.hist = p.hist != 0; return k; }
    k.l2 = a.l2_in_lds ? (a.l2_u16 ? 2 : 1) : 0;
    if (a.k1a_team) { k.family = K1A_TEAM; k.pb = p.np == 256 ? 8 : p.np == 512 ? 9 : 10; k.pair = a.k1a_pair; }
    else { k.family = K1A_TILE; k.nsub = a.k1a_nsub == 2 ? 2 : 1; }
    return k;
}
inline Kernels choose_kernels(const Plan& p, const PassA& a, const sg_config& cfg) {
    Kernels k;
    k.k1a = choose_pass_a(p, a, cfg);
    if (p.variant == 0) {
        // several partitions per CU and room for two tables: the SGPR-capped build lets two workgroups share a CU
        k.k1b_share = p.npb > p.cus && 2 * p.k1b_lds <= kLdsBytes;
        const u32 spt = p.k1b_ht / p.k1b_threads;                      // table slots per thread of the compaction
        k.k1b_u = p.k1b_u == 8 ? 8 : 4;
        if (p.warm || p.narrow) { k.k1b_family = K1B_STREAM; k.k1b_spt = spt >= 4 ? 4 : spt == 2 ? 2 : 1; k.k1b_pack = p.k1b_pack; k.k1b_warm = p.warm != 0; }
        else { k.k1b_family = K1B_MERGE; k.k1b_hist = p.hist != 0; if (k.k1b_hist) k.k1b_u = 4; }
    }
    k.k2_dh = p.dh_g != 0;
    k.k4_split = p.k4_split; k.k4_mfma = p.use_mfma; k.k5_mfma = p.use_mfma; k.k5_form = (int)p.k5_form; k.k5_efeat = (int)p.k5_efeat;
    k.k3_in_form = (int)p.k3_in_form; k.k3_feat_lanes = (int)p.k3_feat_lanes;
    return k;
}

// The instantiations the library holds, per family: one key per kernel, its template arguments in the kernel's own order (pass B's
// last element: share).  servicegraph.hip expands these into its kernel tables; plan_driver plan --domains prints them.
template <size_t N> using Key = std::array<int, N>;
template <size_t... L>
constexpr std::array<Key<sizeof...(L)>, (L * ...)> product(const int (&... v)[L]) {      // every combination of one value per list
    std::array<Key<sizeof...(L)>, (L * ...)> out{};
    for (size_t i = 0; i < out.size(); i++) { size_t r = i, k = 0; ((out[i][k++] = v[r % L], r /= L), ...); }
    return out;
}
template <size_t N, size_t A, size_t B>
constexpr std::array<Key<N>, A + B> concat(const std::array<Key<N>, A>& a, const std::array<Key<N>, B>& b) {
    std::array<Key<N>, A + B> out{};
    for (size_t i = 0; i < A; i++) out[i] = a[i];
    for (size_t i = 0; i < B; i++) out[A + i] = b[i];
    return out;
}
template <size_t N, size_t M>
int find_key(const std::array<Key<N>, M>& dom, const Key<N>& k) { for (size_t i = 0; i < M; i++) if (dom[i] == k) return (int)i; return -1; }

inline constexpr auto kK1aWideKeys = product({0, 1}, {0, 1}, {0, 1});                    // k1a_partition<l2, sharded, hist>
inline constexpr auto kK1aTileKeys = product({0, 1, 2}, {0, 1}, {1, 2});                 // k1a_tile_partition<l2, sharded, nsub>
inline constexpr auto kK1aTeamKeys = product({0, 1, 2}, {0, 1}, {8, 9, 10});             // k1a_team_partition<l2, sharded, 2, 1024, pb>
inline constexpr auto kK1aTeamPairKeys = product({0, 1, 2}, {0, 1}, {8, 9, 10});           // k1a_team_partition<l2, sharded, 2, 1024, pb, 1>: the paired form
inline constexpr auto kK1bMergeKeys = concat(product({4, 8}, {0}, {0, 1}), product({4}, {1}, {0, 1}));   // k1b_merge[_wide]<u, hist>, share
inline constexpr auto kK1bStreamKeys = concat(product({4, 8}, {1, 2, 4}, {0, 1}, {0}, {0, 1}),           // k1b_stream_merge[_wide]<u, spt, pack, wm>, share
                                              product({kK1bWarmU}, {1, 2, 4}, {0, 1}, {1, 2}, {0, 1}));
inline constexpr auto kK4LayerKeys = product({32, 64}, {0, 1}, {0, 1}, {0, 1});          // k4_sage_layer<fi, mfma, proj, threads, split>

// ---- the opt-in stages' device blocks -------------------------------------------------------------------------------------------
// Every opt-in stage behind K5 gets one device block from its sg_set_* call (K7's scratch: at the first selection).  Block cuts it:
// take() hands out offsets in call order, each aligned, and records the piece; the plan keeps the offsets, Block's end as its
// total_bytes and the record as its layout (what the CPU drivers under tests/micro print).  slots() cuts the per-slot region: every
// window slot holds the same pieces in the same order, piece i of slot k at Slots::off + k * Slots::bytes + *SlotPiece::rel.
constexpr u64 kTrendAlign = 256;
inline u64 trend_align(u64 b) { return (b + kTrendAlign - 1) / kTrendAlign * kTrendAlign; }
struct Piece { const char* name; u64 off, bytes; };
struct Slots { u64 off = 0, bytes = 0; };
struct SlotPiece { const char* name; u64 bytes; u64* rel; };
struct Block {
    u64 align = kTrendAlign, end = 0;
    std::vector<Piece> pieces;
    u64 up(u64 b) const { return (b + align - 1) / align * align; }
    u64 take(const char* name, u64 bytes) {
        const u64 off = up(end);
        pieces.push_back({name, off, bytes});
        end = off + bytes;
        return off;
    }
    Slots slots(u32 n, std::initializer_list<SlotPiece> ps) {
        Slots s;
        for (u32 k = 0; k < std::max<u32>(n, 1); k++) {
            const u64 first = up(end);
            for (const SlotPiece& p : ps) { const u64 off = take(p.name, p.bytes); if (!k) *p.rel = off - first; }
            if (!k) { s.off = first; s.bytes = up(end) - first; }
        }
        return s;
    }
};

// K7, the selection (sg_sel.h): its scratch and grids.  Allocated at an engine's first selection: an engine that never selects
// asks for nothing (used = false).  Rows are split into `wgs` contiguous spans of at least 2048 (eight rows per lane of a 256-thread
// workgroup, two such workgroups per CU at 1 M edges); k7_scan scans one count per thread of one 1024-thread workgroup.
constexpr u32 kSelThreads = 256, kSelMaxWgs = 1024, kSelRowsPerWg = 2048, kSelStateWords = 8;
struct SelPlan {
    u32 wgs = 0;                  // workgroups of k7_keys / k7_hist / k7_count / k7_scatter
    u64 key_bytes = 0;            // one u32 key per row: max_edges
    u64 hist_bytes = 0;           // [wgs][256] u32
    u64 blk_bytes = 0;            // [wgs][4] u32
    u64 pair_bytes = 0;           // [SG_SELECT_MAX_K] u64 (top-k)
    u64 state_bytes = 0;          // k7 state words + the selected count (u64)
    u64 scratch_bytes = 0;        // all of the above: what sg_window_select needs
    u64 stage_rows = 0;           // device staging of the host flushes' rows: threshold mode may select every row
    // the scratch's layout, 8-byte aligned: the u64 arrays first (the state piece: the selected count, then the state words)
    u64 pair_off = 0, n_off = 0, state_off = 0, blk_off = 0, hist_off = 0, key_off = 0;
    std::vector<Piece> layout;
};
inline SelPlan plan_select(u64 max_edges, bool used) {
    SelPlan s;
    if (!used) return s;
    s.wgs = (u32)std::max<u64>(1, std::min<u64>(kSelMaxWgs, (max_edges + kSelRowsPerWg - 1) / kSelRowsPerWg));
    s.key_bytes = max_edges * 4;
    s.hist_bytes = (u64)s.wgs * 256 * 4;
    s.blk_bytes = (u64)s.wgs * 4 * 4;
    s.pair_bytes = (u64)SG_SELECT_MAX_K * 8;
    s.state_bytes = kSelStateWords * 4 + 8;
    s.stage_rows = max_edges;
    Block b; b.align = 8;
    s.pair_off = b.take("pairs", s.pair_bytes);
    s.n_off = b.take("state", s.state_bytes); s.state_off = s.n_off + 8;
    s.blk_off = b.take("blk", s.blk_bytes);
    s.hist_off = b.take("hist", s.hist_bytes);
    s.key_off = b.take("keys", s.key_bytes);
    s.scratch_bytes = b.end; s.layout = std::move(b.pieces);
    return s;
}
// An index selection (K7 over rows that are not the edge rows: K9's node rows, K16's workload rows, K14's group edges): the whole
// block of the first one — the host form's staging of stage_rows rows of row_bytes each, the counter block the key pass fills
// (counter_bytes: the engine's, the plan includes no device header), an index array over the rows, then K7's scratch over `rows` keys
struct IndexSelPlan {
    SelPlan sel;
    u64 stage_rows = 0;           // rows the host form's staging holds
    u64 stage_bytes = 0;          // [stage_rows] rows
    u64 ctr_bytes = 0;            // the counter block
    u64 idx_bytes = 0;            // [rows] u32
    u64 sel_bytes = 0;            // sel.scratch_bytes
    u64 stage_off = 0, ctr_off = 0, idx_off = 0, sel_off = 0;
    u64 total_bytes = 0;          // all of it, each piece 256-byte aligned
    std::vector<Piece> layout;
};
inline IndexSelPlan plan_index_select(u64 rows, u64 stage_rows, u64 row_bytes, u64 counter_bytes) {
    IndexSelPlan n;
    n.sel = plan_select(rows, true);
    n.stage_rows = stage_rows;
    n.stage_bytes = trend_align(stage_rows * row_bytes);
    n.ctr_bytes = trend_align(counter_bytes);
    n.idx_bytes = trend_align(rows * 4);
    n.sel_bytes = trend_align(n.sel.scratch_bytes);
    Block b;
    n.stage_off = b.take("stage", n.stage_bytes);
    n.ctr_off = b.take("ctr", n.ctr_bytes);
    n.idx_off = b.take("idx", n.idx_bytes);
    n.sel_off = b.take("sel", n.sel_bytes);
    n.total_bytes = b.end; n.layout = std::move(b.pieces);
    return n;
}
// Node selection (K7 over K9's node rows, k10_keys / k11_keys): over ncap rows, every one of them staged
using NodeSelPlan = IndexSelPlan;
inline NodeSelPlan plan_node_select(u32 ncap, u64 counter_bytes) {
    const u64 NC = std::max<u32>(ncap, 1);
    return plan_index_select(NC, NC, sizeof(sg_node_out), counter_bytes);
}
// k7_sort's LDS: the selected (key, index) pairs padded to a power of two, 8 bytes each
inline size_t select_sort_lds(u32 k) { return (size_t)next_pow2(std::max<u32>(k, 1)) * 8; }

// K8, the per-edge baselines (sg_trend.h): the parameters with their defaults filled in, and the device memory sg_set_trend
// allocates — never sg_create: an engine without the trend asks for nothing.  The merge of B <= max_entries old entries with
// E <= max_edges rows is split into one span per thread of `wgs` 256-thread workgroups, about eight merged elements per thread
// (at most 1024 workgroups: k8_scan scans one count per thread of one 1024-thread workgroup; beyond that the spans grow).
constexpr u32 kTrendThreads = 256, kTrendMaxWgs = 1024, kTrendPerThread = 8, kTrendCtlWords = 8;
constexpr u64 kTrendMaxEntries = 1ull << 31;              // the per-window counts are u32
// SG_OK and *out = p with every 0 replaced by its default, or SG_EINVAL
inline int check_trend(const sg_trend_params& p, u64 max_edges, sg_trend_params* out) {
    if (p.struct_size != sizeof(sg_trend_params) || p.reserved != 0 || p.shift > 10 || p.max_entries > kTrendMaxEntries) return SG_EINVAL;
    sg_trend_params r = p;
    if (!r.shift) r.shift = 4;
    if (!r.warmup) r.warmup = 4;
    if (!r.ttl) r.ttl = 64;
    if (!r.max_entries) r.max_entries = std::min<u64>(kTrendMaxEntries, 2 * std::max<u64>(max_edges, 1));
    if (!r.lat_floor_ns) r.lat_floor_ns = 1000;
    if (!r.err_floor) r.err_floor = 10486;
    *out = r;
    return SG_OK;
}
struct TrendPlan {
    u64 entries = 0;              // max_entries
    u32 wgs = 0;                  // workgroups of the count and write passes (k8_count / k8_write, k10_count / k10_write)
    u64 soa_bytes = 0;            // one baseline buffer: 56 bytes per entry (from_key, to_key, four fp64, n, last)
    u64 ctl_bytes = 0;            // the control block: B per parity, room, statistics
    u64 blk_bytes = 0;            // [wgs][4] u32
    u64 thread_bytes = 0;         // [wgs * 256] per-thread split + counts (16 bytes)
    u64 rows_bytes = 0;           // one window slot's trend rows
    u64 total_bytes = 0;          // two baseline buffers, the scratch and every slot's rows, each 256-byte aligned
    u64 soa_off[2] = {}, ctl_off = 0, blk_off = 0, thread_off = 0;
    Slots slot; u64 slot_rows = 0;
    // inside one baseline buffer, back to back, the 64-bit arrays first (8-byte aligned; the u32 arrays 4): the keys, the four fp64
    // arrays (lat_mean, lat_dev, err_mean, err_dev), n, last
    u64 soa_from_key = 0, soa_to_key = 0, soa_stat[4] = {}, soa_n = 0, soa_last = 0;
    std::vector<Piece> layout, soa_layout;
};
// a baseline of max_entries entries merged with at most `samples` samples a window, `row_bytes` of trend rows per window slot
inline TrendPlan plan_baseline(const sg_trend_params& p, u64 samples, u64 row_bytes, u32 slots) {
    TrendPlan t;
    t.entries = p.max_entries;
    const u64 T = p.max_entries + samples, per_wg = (u64)kTrendThreads * kTrendPerThread;
    t.wgs = (u32)std::max<u64>(1, std::min<u64>(kTrendMaxWgs, (T + per_wg - 1) / per_wg));
    t.soa_bytes = trend_align(p.max_entries * (2 * 8 + 4 * 8 + 2 * 4));
    t.ctl_bytes = trend_align(kTrendCtlWords * 8);
    t.blk_bytes = trend_align((u64)t.wgs * 4 * 4);
    t.thread_bytes = trend_align((u64)t.wgs * kTrendThreads * 16);
    t.rows_bytes = trend_align(row_bytes);
    Block b;
    t.soa_off[0] = b.take("soa0", t.soa_bytes); t.soa_off[1] = b.take("soa1", t.soa_bytes);
    t.ctl_off = b.take("ctl", t.ctl_bytes);
    t.blk_off = b.take("blk", t.blk_bytes);
    t.thread_off = b.take("thread", t.thread_bytes);
    t.slot = b.slots(slots, {{"rows", t.rows_bytes, &t.slot_rows}});
    t.total_bytes = b.end; t.layout = std::move(b.pieces);
    Block q; q.align = 4;
    const u64 C = p.max_entries;
    t.soa_from_key = q.take("from_key", C * 8); t.soa_to_key = q.take("to_key", C * 8);
    const char* const stat[4] = {"lat_mean", "lat_dev", "err_mean", "err_dev"};
    for (int k = 0; k < 4; k++) t.soa_stat[k] = q.take(stat[k], C * 8);
    t.soa_n = q.take("n", C * 4); t.soa_last = q.take("last", C * 4);
    t.soa_layout = std::move(q.pieces);
    return t;
}
// K8: the window's edge rows, [max_edges] sg_edge_trend per slot
inline TrendPlan plan_trend(u64 max_edges, u32 slots, const sg_trend_params& p) {
    return plan_baseline(p, max_edges, std::max<u64>(max_edges, 1) * sizeof(sg_edge_trend), slots);
}

// K8's vanished list (sg_set_vanished): the parameters with their defaults filled in against the trend's resolved parameters, and
// the device memory sg_set_vanished allocates — never sg_create or sg_set_trend.  The per-thread and per-workgroup counts are
// scratch of k8_count_v / k8_scan_v / k8_write_v (the trend's grid); each window slot keeps its list and its count.
constexpr u32 kVanishedDefaultRows = 65536;
inline int check_vanished(const sg_vanished_params& p, const sg_trend_params& trend, sg_vanished_params* out) {
    if (p.struct_size != sizeof(sg_vanished_params)) return SG_EINVAL;
    sg_vanished_params r = p;
    if (!r.silent_windows) r.silent_windows = 1;
    if (!r.min_seen) r.min_seen = trend.warmup;
    if (!r.max_rows) r.max_rows = (u32)std::min<u64>(kVanishedDefaultRows, trend.max_entries);
    if (r.silent_windows >= trend.ttl || r.max_rows > trend.max_entries) return SG_EINVAL;
    *out = r;
    return SG_OK;
}
struct VanishedPlan {
    u64 rows = 0;                 // max_rows
    u64 thread_bytes = 0;         // [wgs * 256] u32 per-thread counts
    u64 blk_bytes = 0;            // [wgs] u32 per-workgroup counts
    u64 list_bytes = 0;           // one window slot's list: [max_rows] sg_edge_vanished
    u64 count_bytes = 0;          // one window slot's count (u64)
    u64 total_bytes = 0;          // the scratch and every slot's list and count, each 256-byte aligned
    u64 thread_off = 0, blk_off = 0;
    Slots slot; u64 slot_list = 0, slot_count = 0;
    std::vector<Piece> layout;
};
inline VanishedPlan plan_vanished(const TrendPlan& t, u32 slots, const sg_vanished_params& p) {
    VanishedPlan v;
    v.rows = p.max_rows;
    v.thread_bytes = trend_align((u64)t.wgs * kTrendThreads * 4);
    v.blk_bytes = trend_align((u64)t.wgs * 4);
    v.list_bytes = trend_align(std::max<u64>(p.max_rows, 1) * sizeof(sg_edge_vanished));
    v.count_bytes = trend_align(8);
    Block b;
    v.thread_off = b.take("thread", v.thread_bytes);
    v.blk_off = b.take("blk", v.blk_bytes);
    v.slot = b.slots(slots, {{"list", v.list_bytes, &v.slot_list}, {"count", v.count_bytes, &v.slot_count}});
    v.total_bytes = b.end; v.layout = std::move(b.pieces);
    return v;
}

// K9, the node rollup (sg_nodes.h): the device memory sg_set_nodes allocates — never sg_create.  Nodes are keyed by an id below
// ncap = max_known + max_labels + max_obip.  k9_out takes chunks of 2048 rows (256 threads x 8); k9_in_part a grid of node ranges
// of 2048 (128 KiB of LDS each) x row slices — about 32 K rows per slice, at most 16 slices, as k3_in_part; k9_count / k9_write
// one 256-thread workgroup per block of node_per nodes, at most 1024 blocks (k9_scan scans one count per thread).
constexpr u32 kNodesThreads = 256, kNodesChunk = 2048, kNodesRangeNodes = 2048, kNodesMaxSlices = 16, kNodesSliceRows = 32768,
              kNodesMaxWgs = 1024;
constexpr u64 kNodesSideBytes = 64;       // one side of a node: a table entry, an LDS entry, a partial
// The rollup exists in two key spaces — K9's node ids and K16's group keys (below) — with one plan: plan_rollup sizes and lays out
// the block of either from the row capacity of the input, the key count, the rows a window slot holds and a cap on the in side's grid.
struct NodesPlan {
    u32 ncap = 0;                 // K9's node id space (K9's key count; K16's keys are max_groups + ncap)
    u32 out_wgs = 0;              // workgroups of the out side: chunks of max_edges
    u32 ranges = 0, slices = 0;   // the in side's grid = ranges x slices
    u32 node_wgs = 0, node_per = 0;   // the count / write passes: workgroups, keys per workgroup (a multiple of 256)
    u64 dst_bytes = 0;            // [max_edges] u32 destination key per row
    u64 table_bytes = 0;          // one side's table: [keys] x 64 bytes (out and in: two of them)
    u64 part_bytes = 0;           // [ranges][slices][2048] x 64 bytes
    u64 blk_bytes = 0;            // [2][1024] u32
    u64 rows_bytes = 0;           // one window slot's rows: [rows] sg_node_out
    u64 count_bytes = 0;          // one window slot's row count (u64)
    u64 lds_bytes = 0;            // the in side's dynamic LDS
    u64 total_bytes = 0;          // the scratch and every slot's rows and count, each 256-byte aligned
    u64 table_off[2] = {}, part_off = 0, dst_off = 0, blk_off = 0;   // (table_off: out, in)
    Slots slot; u64 slot_rows = 0, slot_count = 0;
    std::vector<Piece> layout;
};
// max_in_wgs: at most about that many workgroups on the in side (0: no cap) — a range's workgroups scan every row of their slice
inline void plan_rollup(NodesPlan& n, u64 max_edges, u64 keys, u64 rows, u32 max_in_wgs, u32 slots) {
    const u64 ME = std::max<u64>(max_edges, 1), NK = std::max<u64>(keys, 1);
    n.out_wgs = (u32)((ME + kNodesChunk - 1) / kNodesChunk);
    n.ranges = (u32)((NK + kNodesRangeNodes - 1) / kNodesRangeNodes);
    n.slices = (u32)std::max<u64>(1, std::min<u64>(kNodesMaxSlices, (ME + kNodesSliceRows - 1) / kNodesSliceRows));
    if (max_in_wgs) n.slices = std::min<u32>(n.slices, std::max<u32>(1, max_in_wgs / n.ranges));
    n.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kNodesMaxWgs, (NK + kNodesThreads - 1) / kNodesThreads));
    const u64 per = (NK + n.node_wgs - 1) / n.node_wgs;
    n.node_per = (u32)((per + kNodesThreads - 1) / kNodesThreads * kNodesThreads);
    n.node_wgs = (u32)((NK + n.node_per - 1) / n.node_per);           // (the rounding can leave the last blocks without keys)
    n.dst_bytes = trend_align(ME * 4);
    n.table_bytes = trend_align(NK * kNodesSideBytes);
    n.part_bytes = trend_align((u64)n.ranges * n.slices * kNodesRangeNodes * kNodesSideBytes);
    n.blk_bytes = trend_align(2ull * kNodesMaxWgs * 4);
    n.rows_bytes = trend_align(std::max<u64>(rows, 1) * sizeof(sg_node_out));
    n.count_bytes = trend_align(8);
    n.lds_bytes = (u64)kNodesRangeNodes * kNodesSideBytes;
    Block b;
    n.table_off[0] = b.take("table_out", n.table_bytes); n.table_off[1] = b.take("table_in", n.table_bytes);
    n.part_off = b.take("part", n.part_bytes);
    n.dst_off = b.take("dst", n.dst_bytes);
    n.blk_off = b.take("blk", n.blk_bytes);
    n.slot = b.slots(slots, {{"rows", n.rows_bytes, &n.slot_rows}, {"count", n.count_bytes, &n.slot_count}});
    n.total_bytes = b.end; n.layout = std::move(b.pieces);
}
inline NodesPlan plan_nodes(u64 max_edges, u32 ncap, u32 slots) {
    NodesPlan n;
    n.ncap = ncap;
    plan_rollup(n, max_edges, ncap, ncap, 0, slots);
    return n;
}

// K10, the per-node baselines (sg_node_trend.h): K8's parameters and memory over the node rows — sg_set_node_trend allocates it,
// never sg_create or sg_set_nodes.  A window has at most 2 x ncap samples (two sides per node row); max_entries defaults to
// 4 x ncap (two sides, and OBIP nodes change from window to window).  The grid is K8's rule over B + 2 x ncap merged elements.
// Node selection reuses K7's plan over ncap rows (plan_select(ncap)) and its own index / row staging of ncap each.
inline int check_node_trend(const sg_trend_params& p, u32 ncap, sg_trend_params* out) {
    if (p.struct_size != sizeof(sg_trend_params)) return SG_EINVAL;
    sg_trend_params q = p;
    if (!q.max_entries) q.max_entries = std::min<u64>(kTrendMaxEntries, 4 * std::max<u64>(ncap, 1));
    return check_trend(q, 0, out);
}
// K10: two samples per node row, [ncap] sg_node_trend per slot.  The node plan is K8's type; NodeTrendPlan names it for the CPU
// driver tests/micro/plan_driver.cpp, stage node_trend.
using NodeTrendPlan = TrendPlan;
inline TrendPlan plan_node_trend(u32 ncap, u32 slots, const sg_trend_params& p) {
    return plan_baseline(p, 2 * (u64)ncap, std::max<u64>(ncap, 1) * sizeof(sg_node_trend), slots);
}

// K11, the culprit ranking (sg_rank.h): parameters and the device memory sg_set_rank allocates — never sg_create or sg_set_nodes.
// Work is in K9's node-key space (ncap).  k11_edge takes a grid of node ranges of 16 384 (128 KiB of u64 accumulators in LDS) x
// row slices — about 32 K rows per slice, at most 32 slices and at most 256 workgroups (each writes a 128 KiB partial per pass,
// and a range's workgroups scan every row of their slice: many ranges take fewer slices); k11_prep and k11_node run a grid-stride
// grid of 256-thread workgroups, at most 1024 (k11_node sums one seed sum per k11_prep workgroup).  The scratch is shared by the
// window slots; each slot keeps its rank rows; one staging block serves sg_window_rank's index form and sg_window_rank_top.
constexpr u32 kRankThreads = 256, kRankRangeNodes = 16384, kRankMaxSlices = 32, kRankSliceRows = 32768, kRankMaxEdgeWgs = 256,
              kRankMaxWgs = 1024, kRankMaxIters = 64, kRankDefaultIters = 20, kRankDefaultDamping = 218;
// SG_OK and *out = p with every 0 replaced by its default, or SG_EINVAL
inline int check_rank(const sg_rank_params& p, sg_rank_params* out) {
    if (p.struct_size != sizeof(sg_rank_params) || p.reserved != 0 || p.iters > kRankMaxIters || p.damping_q8 > 255 ||
        p.seed > SG_RANK_SEED_UNIFORM) return SG_EINVAL;
    sg_rank_params r = p;
    if (!r.iters) r.iters = kRankDefaultIters;
    if (!r.damping_q8) r.damping_q8 = kRankDefaultDamping;
    *out = r;
    return SG_OK;
}
// The ranking exists in two spaces — K11's over the node keys and K17's over the workload rows (below).  What their blocks share
// is sized and laid out once, by plan_rank_block: four u64 arrays by node (W, R, base, t), the edge pass's partials, the seed sums,
// the staging of the index reads and every slot's rank rows.  The grids are each plan's own: their rules differ.
struct RankBlock {
    u32 ranges = 0, slices = 0;   // the edge pass's grid = ranges x slices
    u32 prep_wgs = 0;             // the prep pass: grid-stride over the rows it reads
    u32 node_wgs = 0;             // the node pass: grid-stride over the node arrays
    u64 node_bytes = 0;           // one per-node u64 array (W, R, base, t: four of them)
    u64 part_bytes = 0;           // [ranges][slices][a range's nodes] u64
    u64 seed_bytes = 0;           // [1024] u64
    u64 stage_bytes = 0;          // one sg_node_rank per node: staging
    u64 stage_idx_bytes = 0;      // one u32 per node: staging
    u64 rows_bytes = 0;           // one window slot's rank rows: one sg_node_rank per node
    u64 lds_bytes = 0;            // the edge pass's dynamic LDS: a range of u64 accumulators
    u64 total_bytes = 0;          // the scratch, the staging and every slot's rows, each 256-byte aligned
    u64 node_off[4] = {}, part_off = 0, seed_off = 0, stage_off = 0, stage_idx_off = 0;   // (node_off: W, R, base, t)
    Slots slot; u64 slot_rows = 0;
    std::vector<Piece> layout;
};
// r.ranges and r.slices set: the sizes over `nodes` node keys or rows in ranges of range_nodes, and the block — the node arrays, the
// partials and the seed sums, then the plan's own per-row arrays (own(b) takes them), the staging and the slots
template <class Own>
inline void plan_rank_block(RankBlock& r, u64 nodes, u32 range_nodes, u32 slots, Own own) {
    r.node_bytes = trend_align(nodes * 8);
    r.part_bytes = trend_align((u64)r.ranges * r.slices * range_nodes * 8);
    r.seed_bytes = trend_align((u64)kRankMaxWgs * 8);
    r.stage_bytes = trend_align(nodes * sizeof(sg_node_rank));
    r.stage_idx_bytes = trend_align(nodes * 4);
    r.rows_bytes = trend_align(nodes * sizeof(sg_node_rank));
    r.lds_bytes = (u64)range_nodes * 8;
    Block b;
    const char* const node[4] = {"W", "R", "base", "t"};
    for (int k = 0; k < 4; k++) r.node_off[k] = b.take(node[k], r.node_bytes);
    r.part_off = b.take("part", r.part_bytes);
    r.seed_off = b.take("seed", r.seed_bytes);
    own(b);
    r.stage_off = b.take("stage", r.stage_bytes);
    r.stage_idx_off = b.take("stage_idx", r.stage_idx_bytes);
    r.slot = b.slots(slots, {{"rows", r.rows_bytes, &r.slot_rows}});
    r.total_bytes = b.end; r.layout = std::move(b.pieces);
}
struct RankPlan : RankBlock {     // (k11_edge, k11_prep over max(max_edges, ncap), k11_node over ncap)
    typedef u32 Weight;           // an element of w
    u32 ncap = 0;
    u64 row_bytes = 0;            // one per-row u32 array [max_edges] (src, dst, w: three of them)
    u64 row_off[3] = {};          // (src, dst, w)
};
inline RankPlan plan_rank(u64 max_edges, u32 ncap, u32 slots) {
    RankPlan r;
    const u64 ME = std::max<u64>(max_edges, 1), NC = std::max<u32>(ncap, 1);
    r.ncap = ncap;
    r.ranges = (u32)((NC + kRankRangeNodes - 1) / kRankRangeNodes);
    r.slices = (u32)std::max<u64>(1, std::min<u64>(kRankMaxSlices, (ME + kRankSliceRows - 1) / kRankSliceRows));
    r.slices = std::max<u32>(1, std::min<u32>(r.slices, kRankMaxEdgeWgs / std::max<u32>(r.ranges, 1)));
    r.prep_wgs = (u32)std::max<u64>(1, std::min<u64>(kRankMaxWgs, (std::max(ME, NC) + 4 * kRankThreads - 1) / (4 * kRankThreads)));
    r.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kRankMaxWgs, (NC + kRankThreads - 1) / kRankThreads));
    r.row_bytes = trend_align(ME * 4);
    plan_rank_block(r, NC, kRankRangeNodes, slots, [&r](Block& b) {
        const char* const row[3] = {"src", "dst", "w"};
        for (int k = 0; k < 3; k++) r.row_off[k] = b.take(row[k], r.row_bytes);
    });
    return r;
}

// K12, the incidents (sg_incident.h): parameters and the device memory sg_set_incidents allocates — never sg_create or
// sg_set_nodes.  Work is in K9's node-key space (ncap): five u32 arrays by node key (parent, flag, label, number, incident) and the
// max fields' keys by incident (a window has at most as many incidents as node rows) are scratch shared by the window slots, with
// the head counts k9_scan scans.  k12_label / k12_number take one 256-thread workgroup per block of node_per node rows, at most
// 1024 blocks (K9's rule); k12_init, k12_nodes and k12_finish run a grid-stride grid over ncap; k12_hook one over max_edges, at
// most 1024 workgroups; k12_rows at most 256 (every workgroup adds its LDS table to the incidents once: fewer workgroups, fewer
// device atomics on one incident).  Each slot keeps its incident rows, their count and the incident per node row; one staging
// block serves sg_window_node_incident's index form.
constexpr u32 kIncThreads = 256, kIncMaxWgs = 1024, kIncMaxRowWgs = 256, kIncRowsPerThread = 4;
constexpr u64 kIncKeysBytes = 24;         // worst, top, rmax
inline int check_incidents(const sg_incident_params& p, sg_incident_params* out) {
    if (p.struct_size != sizeof(sg_incident_params) || p.reserved != 0 || p.by > SG_SEL_ERR_DEV) return SG_EINVAL;
    *out = p;
    return SG_OK;
}
// The incidents exist in two spaces — K12's over the node keys and K18's over the workload rows (below).  What their plans share
// is sized and laid out once, by plan_incident_block: the grids but the *_nodes pass's, the max fields' keys by incident, the head
// counts, the staging of the index reads and every slot's incident rows, count and incident per node.
struct IncidentBlock {
    u32 node_wgs = 0, node_per = 0;   // the label / number passes: workgroups, nodes per workgroup (a multiple of 256)
    u32 grid_wgs = 0;             // the init and finish passes (and k12_nodes): grid-stride over the nodes
    u32 hook_wgs = 0;             // the hook pass: grid-stride over max_edges
    u32 row_wgs = 0;              // the rows pass: grid-stride over max_edges (and the nodes)
    u64 keys_bytes = 0;           // one node x 24 bytes: the max fields' keys per incident
    u64 blk_bytes = 0;            // [2][1024] u32
    u64 stage_bytes = 0;          // one u32 per node: staging, and as much for the index (two of them)
    u64 rows_bytes = 0;           // one window slot's incidents: one sg_incident_out per node
    u64 count_bytes = 0;          // one window slot's incident count (u64)
    u64 node_inc_bytes = 0;       // one window slot's incident per node: one u32 each
    u64 total_bytes = 0;          // the scratch, the staging and every slot's buffers, each 256-byte aligned
    u64 keys_off = 0, blk_off = 0, stage_off = 0, stage_idx_off = 0;
    Slots slot; u64 slot_rows = 0, slot_count = 0, slot_node_inc = 0;
    std::vector<Piece> layout;
};
// the grids and sizes over `nodes` node keys or rows, and the block: the keys, then the plan's own per-node and per-edge arrays
// (own(b) takes them), the head counts, the staging and the slots
template <class Own>
inline void plan_incident_block(IncidentBlock& r, u64 max_edges, u64 nodes, u32 slots, Own own) {
    const u64 ME = std::max<u64>(max_edges, 1), NC = nodes;
    r.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kIncMaxWgs, (NC + kIncThreads - 1) / kIncThreads));
    const u64 per = (NC + r.node_wgs - 1) / r.node_wgs;
    r.node_per = (u32)((per + kIncThreads - 1) / kIncThreads * kIncThreads);
    r.node_wgs = (u32)((NC + r.node_per - 1) / r.node_per);
    r.grid_wgs = (u32)std::max<u64>(1, std::min<u64>(kIncMaxWgs, (NC + kIncThreads - 1) / kIncThreads));
    const u64 row_blocks = (ME + (u64)kIncRowsPerThread * kIncThreads - 1) / ((u64)kIncRowsPerThread * kIncThreads);
    r.hook_wgs = (u32)std::max<u64>(1, std::min<u64>(kIncMaxWgs, row_blocks));
    r.row_wgs = (u32)std::max<u64>(1, std::min<u64>(kIncMaxRowWgs, row_blocks));
    r.keys_bytes = trend_align(NC * kIncKeysBytes);
    r.blk_bytes = trend_align(2ull * kIncMaxWgs * 4);
    r.stage_bytes = trend_align(NC * 4);
    r.rows_bytes = trend_align(NC * sizeof(sg_incident_out));
    r.count_bytes = trend_align(8);
    r.node_inc_bytes = trend_align(NC * 4);
    Block b;
    r.keys_off = b.take("keys", r.keys_bytes);
    own(b);
    r.blk_off = b.take("blk", r.blk_bytes);
    r.stage_off = b.take("stage", r.stage_bytes); r.stage_idx_off = b.take("stage_idx", r.stage_bytes);
    r.slot = b.slots(slots, {{"rows", r.rows_bytes, &r.slot_rows}, {"count", r.count_bytes, &r.slot_count},
                             {"node_inc", r.node_inc_bytes, &r.slot_node_inc}});
    r.total_bytes = b.end; r.layout = std::move(b.pieces);
}
struct IncidentPlan : IncidentBlock {
    u32 ncap = 0;
    u64 key_bytes = 0;            // one per-node-key u32 array [ncap] (parent, flag, lab, num, kinc: five of them)
    u64 key_off[5] = {};          // (parent, flag, lab, num, kinc)
};
inline IncidentPlan plan_incidents(u64 max_edges, u32 ncap, u32 slots) {
    IncidentPlan r;
    const u64 NC = std::max<u32>(ncap, 1);
    r.ncap = ncap;
    r.key_bytes = trend_align(NC * 4);
    plan_incident_block(r, max_edges, NC, slots, [&r](Block& b) {
        const char* const key[5] = {"parent", "flag", "lab", "num", "kinc"};
        for (int k = 0; k < 5; k++) r.key_off[k] = b.take(key[k], r.key_bytes);
    });
    return r;
}

// K13, the tracks (sg_track.h): parameters and the device memory sg_set_tracks allocates — never sg_create, sg_set_nodes or
// sg_set_incidents.  Kept across windows: the members, two u32 arrays by anchor key (max_known + max_labels), the track table
// twice ([max_tracks] sg_track_entry: one buffer is read and the other written per window) and its counters twice.  Scratch shared
// by the window slots: six u32 arrays [ncap] (cand, kept, moved, joined, pos by incident; t_v by node row), the claim words
// [max_tracks] u64 and the workgroup counts k13_scan scans.  k13_count / k13_write take one 256-thread workgroup per span of `per`
// incidents and table entries, at most 1024 spans; k13_init runs a grid-stride grid over max(ncap, max_tracks); k13_claim and
// k13_members one over ncap.  The folding passes k13_look and k13_fold take kTrkFoldRounds rounds of 256 node rows per workgroup:
// every workgroup adds its LDS table to the incidents once, so fewer workgroups mean fewer device atomics on one incident's words (an
// all-red config-3 window: 8 workgroups, not 59), and a workgroup can meet more distinct incidents than its table has slots, which
// then go to device memory directly.  Each slot keeps its sg_incident_track rows, its ended list and the list's count.
constexpr u32 kTrkThreads = 256, kTrkMaxWgs = 1024, kTrkBlkWords = 7 * 1024, kTrkFoldRounds = 8;
constexpr u64 kTrkStateBytes = 24;        // entries, next_id, opened, dropped
inline int check_tracks(const sg_track_params& p, u32 ncap, sg_track_params* out) {
    if (p.struct_size != sizeof(sg_track_params) || p.reserved != 0 || p.quiet_windows > SG_TRACK_MAX_QUIET) return SG_EINVAL;
    *out = p;
    if (!p.max_tracks) {
        const u64 all = (u64)(p.quiet_windows + 1) * std::max<u32>(ncap, 1);
        if (all > 0x7FFFFFFFull) return SG_EINVAL;                    // (ids and positions are u32)
        out->max_tracks = (u32)all;
    }
    return SG_OK;
}
struct TrackPlan {
    u32 ncap = 0, anchors = 0, max_tracks = 0;
    u32 wgs = 0, per = 0;         // k13_count / k13_write: workgroups, incidents and entries per workgroup (a multiple of 256)
    u32 init_wgs = 0;             // k13_init: grid-stride over max(ncap, max_tracks)
    u32 node_wgs = 0;             // k13_claim, k13_members: grid-stride over ncap
    u32 fold_wgs = 0;             // k13_look, k13_fold: grid-stride over ncap, kTrkFoldRounds rounds a workgroup
    u64 member_bytes = 0;         // one member array [anchors] u32 (track, last: two of them)
    u64 table_bytes = 0;          // one table buffer [max_tracks] sg_track_entry (two of them)
    u64 state_bytes = 0;          // one copy of the counters (two of them)
    u64 inc_bytes = 0;            // one scratch u32 array [ncap] (six of them)
    u64 claim_bytes = 0;          // [max_tracks] u64
    u64 blk_bytes = 0;            // [7][1024] u32
    u64 rows_bytes = 0;           // one window slot's rows: [ncap] sg_incident_track
    u64 ended_bytes = 0;          // one window slot's ended list: [ncap] sg_track_entry
    u64 count_bytes = 0;          // one window slot's ended count (u64)
    u64 total_bytes = 0;          // the state, the scratch and every slot's buffers, each 256-byte aligned
    u64 member_off[2] = {}, table_off[2] = {}, state_off[2] = {}, inc_off[6] = {}, claim_off = 0, blk_off = 0;   // (member_off: track, last; inc_off: cand, kept, moved, joined, pos, tv)
    Slots slot; u64 slot_rows = 0, slot_ended = 0, slot_count = 0;
    std::vector<Piece> layout;
};
// the tracks over rows of capacity ncap whose anchor keys are [0, anchors): K13's (plan_tracks) and K19's (plan_group_tracks)
inline TrackPlan plan_track_block(u64 anchors, u32 ncap, u32 max_tracks, u32 slots) {
    TrackPlan r;
    const u64 NC = std::max<u32>(ncap, 1), MT = std::max<u32>(max_tracks, 1), span = std::max(NC, MT);
    r.ncap = ncap; r.anchors = (u32)anchors; r.max_tracks = max_tracks;
    r.wgs = (u32)std::max<u64>(1, std::min<u64>(kTrkMaxWgs, (span + kTrkThreads - 1) / kTrkThreads));
    const u64 per = (span + r.wgs - 1) / r.wgs;
    r.per = (u32)((per + kTrkThreads - 1) / kTrkThreads * kTrkThreads);
    r.wgs = (u32)((span + r.per - 1) / r.per);
    r.init_wgs = (u32)std::max<u64>(1, std::min<u64>(kTrkMaxWgs, (span + kTrkThreads - 1) / kTrkThreads));
    r.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kTrkMaxWgs, (NC + kTrkThreads - 1) / kTrkThreads));
    const u64 fold_rows = (u64)kTrkFoldRounds * kTrkThreads;
    r.fold_wgs = (u32)std::max<u64>(1, std::min<u64>(kTrkMaxWgs, (NC + fold_rows - 1) / fold_rows));
    r.member_bytes = trend_align(std::max<u64>(anchors, 1) * 4);
    r.table_bytes = trend_align(MT * sizeof(sg_track_entry));
    r.state_bytes = trend_align(kTrkStateBytes);
    r.inc_bytes = trend_align(NC * 4);
    r.claim_bytes = trend_align(MT * 8);
    r.blk_bytes = trend_align((u64)kTrkBlkWords * 4);
    r.rows_bytes = trend_align(NC * sizeof(sg_incident_track));
    r.ended_bytes = trend_align(NC * sizeof(sg_track_entry));
    r.count_bytes = trend_align(8);
    Block b;
    const char* const inc[6] = {"cand", "kept", "moved", "joined", "pos", "tv"};
    r.member_off[0] = b.take("mtrack", r.member_bytes); r.member_off[1] = b.take("mlast", r.member_bytes);
    r.table_off[0] = b.take("table0", r.table_bytes); r.table_off[1] = b.take("table1", r.table_bytes);
    r.state_off[0] = b.take("state0", r.state_bytes); r.state_off[1] = b.take("state1", r.state_bytes);
    for (int k = 0; k < 6; k++) r.inc_off[k] = b.take(inc[k], r.inc_bytes);
    r.claim_off = b.take("claim", r.claim_bytes);
    r.blk_off = b.take("blk", r.blk_bytes);
    r.slot = b.slots(slots, {{"rows", r.rows_bytes, &r.slot_rows}, {"ended", r.ended_bytes, &r.slot_ended},
                             {"ended_count", r.count_bytes, &r.slot_count}});
    r.total_bytes = b.end; r.layout = std::move(b.pieces);
    return r;
}
inline TrackPlan plan_tracks(u32 max_known, u32 max_labels, u32 ncap, u32 max_tracks, u32 slots) {
    return plan_track_block(max_known + max_labels, ncap, max_tracks, slots);
}

// K14, the groups (sg_group.h): parameters and the device memory sg_set_groups allocates — never sg_create.  The key of a row is
// gk(from) << kb | gk(to) with kb = bits(GK - 1), GK = max_groups + ncap: 32 bits wide while 2 kb <= 32 (config 3: 15 + 15), else 64;
// it is sorted in passes = ceil(2 kb / 8) stable radix passes over tiles of 4096 positions.  Scratch shared by the window slots: the
// keys and the indices twice (ping-pong), the digit counts [256][tiles], the group map [max_known], per fold chunk of 2048 positions
// its head count, two 80-byte partials and a meta word, the head counts k9_scan scans (k14_heads: cpw chunks per workgroup, at most
// 1024 workgroups), and the staging of sg_window_row_group's index form.  Each slot keeps its group edges [max_edges], row_group,
// perm and the count.
constexpr u32 kGrpThreads = 256, kGrpTile = 4096, kGrpChunk = 2048, kGrpMaxWgs = 1024, kGrpKeyRows = 1024, kGrpStage = 65536;
constexpr u64 kGrpEdgeBytes = 80, kGrpMaxGroups = 1ull << 30;
// SG_OK and *out = p with max_groups 0 replaced by max_known, or SG_EINVAL
inline int check_groups(const sg_group_params& p, u32 max_known, u32 world, sg_group_params* out) {
    if (world > 1 || p.struct_size != sizeof(sg_group_params) || p.reserved[0] != 0 || p.reserved[1] != 0 || p.max_groups > kGrpMaxGroups) return SG_EINVAL;
    *out = p;
    if (!p.max_groups) out->max_groups = max_known;
    return SG_OK;
}
inline u32 bits_of(u64 x) { u32 b = 0; while (x) { b++; x >>= 1; } return b; }
struct GroupPlan {
    u32 max_groups = 0;
    u64 gk = 0;                   // GK = max_groups + ncap: every group key is below it
    u32 kb = 0;                   // bits(GK - 1), at least 1
    u32 key_bytes = 0;            // 4 while 2 kb <= 32, else 8
    u32 passes = 0;               // ceil(2 kb / 8)
    u32 tiles = 0;                // sort tiles of max_edges: the grid of k14_hist / k14_scatter
    u32 key_wgs = 0;              // k14_keys: 1024 rows a workgroup
    u32 chunks = 0;               // fold chunks of max_edges: the grid of k14_fold
    u32 cpw = 0, heads_wgs = 0;   // k14_heads: chunks per workgroup, workgroups (<= 1024)
    u32 stitch_wgs = 0;           // k14_stitch: one thread per chunk
    u64 keys_bytes = 0;           // one key buffer [max_edges] (two of them)
    u64 idx_bytes = 0;            // one u32 array [max_edges]: an index buffer (two), a slot's row_group, a slot's perm
    u64 map_bytes = 0;            // [max_known] u32
    u64 hist_bytes = 0;           // [256][tiles] u32
    u64 chunkcnt_bytes = 0;       // [chunks] u32
    u64 part_bytes = 0;           // [chunks][2] x 80 bytes
    u64 meta_bytes = 0;           // [chunks] x 8 bytes
    u64 blk_bytes = 0;            // [2][1024] u32
    u64 stage_bytes = 0;          // [65536] u32 (the gathered values, the index: two of them)
    u64 rows_bytes = 0;           // one window slot's group edges: [max_edges] sg_group_edge
    u64 count_bytes = 0;          // one window slot's group edge count (u64)
    u64 total_bytes = 0;          // the scratch, the staging and every slot's buffers, each 256-byte aligned
    u64 keys_off[2] = {}, idx_off[2] = {}, map_off = 0, hist_off = 0, chunkcnt_off = 0, part_off = 0, meta_off = 0, blk_off = 0,
        stage_off = 0, stage_idx_off = 0;
    Slots slot; u64 slot_rows = 0, slot_count = 0, slot_row_group = 0, slot_perm = 0;
    std::vector<Piece> layout;
};
inline GroupPlan plan_groups(u64 max_edges, u32 max_known, u32 ncap, u32 max_groups, u32 slots) {
    GroupPlan r;
    const u64 ME = std::max<u64>(max_edges, 1);
    r.max_groups = max_groups;
    r.gk = (u64)max_groups + ncap;
    r.kb = std::max<u32>(1, bits_of(r.gk ? r.gk - 1 : 0));
    r.key_bytes = 2 * r.kb <= 32 ? 4 : 8;
    r.passes = (2 * r.kb + 7) / 8;
    r.tiles = (u32)((ME + kGrpTile - 1) / kGrpTile);
    r.key_wgs = (u32)((ME + kGrpKeyRows - 1) / kGrpKeyRows);
    r.chunks = (u32)((ME + kGrpChunk - 1) / kGrpChunk);
    r.cpw = (r.chunks + kGrpMaxWgs - 1) / kGrpMaxWgs;
    r.heads_wgs = (r.chunks + r.cpw - 1) / r.cpw;
    r.stitch_wgs = (r.chunks + kGrpThreads - 1) / kGrpThreads;
    r.keys_bytes = trend_align(ME * r.key_bytes);
    r.idx_bytes = trend_align(ME * 4);
    r.map_bytes = trend_align(std::max<u64>(max_known, 1) * 4);
    r.hist_bytes = trend_align(256ull * r.tiles * 4);
    r.chunkcnt_bytes = trend_align((u64)r.chunks * 4);
    r.part_bytes = trend_align((u64)r.chunks * 2 * kGrpEdgeBytes);
    r.meta_bytes = trend_align((u64)r.chunks * 8);
    r.blk_bytes = trend_align(2ull * kGrpMaxWgs * 4);
    r.stage_bytes = trend_align((u64)kGrpStage * 4);
    r.rows_bytes = trend_align(ME * kGrpEdgeBytes);
    r.count_bytes = trend_align(8);
    Block b;
    r.keys_off[0] = b.take("keys0", r.keys_bytes); r.keys_off[1] = b.take("keys1", r.keys_bytes);
    r.idx_off[0] = b.take("idx0", r.idx_bytes); r.idx_off[1] = b.take("idx1", r.idx_bytes);
    r.map_off = b.take("map", r.map_bytes);
    r.hist_off = b.take("hist", r.hist_bytes);
    r.chunkcnt_off = b.take("chunkcnt", r.chunkcnt_bytes);
    r.part_off = b.take("part", r.part_bytes);
    r.meta_off = b.take("meta", r.meta_bytes);
    r.blk_off = b.take("blk", r.blk_bytes);
    r.stage_off = b.take("stage", r.stage_bytes); r.stage_idx_off = b.take("stage_idx", r.stage_bytes);
    r.slot = b.slots(slots, {{"rows", r.rows_bytes, &r.slot_rows}, {"count", r.count_bytes, &r.slot_count},
                             {"row_group", r.idx_bytes, &r.slot_row_group}, {"perm", r.idx_bytes, &r.slot_perm}});
    r.total_bytes = b.end; r.layout = std::move(b.pieces);
    return r;
}

// K15, the workload baselines (sg_group_trend.h): K8's parameters and memory over the group edges — sg_set_group_trend allocates
// it, never sg_create or sg_set_groups.  A window has at most max_edges group edges, one sample each; max_entries defaults to K8's
// 2 x max_edges.  The grid is K8's rule over B + max_edges merged elements; the vanished list is plan_vanished over this plan.
inline int check_group_trend(const sg_trend_params& p, u64 max_edges, sg_trend_params* out) {
    if (p.struct_size != sizeof(sg_trend_params)) return SG_EINVAL;
    sg_trend_params q = p;
    if (!q.max_entries) q.max_entries = std::min<u64>(kTrendMaxEntries, 2 * std::max<u64>(max_edges, 1));
    return check_trend(q, max_edges, out);
}
// K15: one sample per group edge, [max_edges] sg_edge_trend per slot.  GroupTrendPlan names K8's type for the CPU driver
// tests/micro/plan_driver.cpp, stage group_trend.
using GroupTrendPlan = TrendPlan;
inline TrendPlan plan_group_trend(u64 max_edges, u32 slots, const sg_trend_params& p) {
    return plan_baseline(p, max_edges, std::max<u64>(max_edges, 1) * sizeof(sg_edge_trend), slots);
}
// Selection over group edges (K7 over K14's rows, k15_keys): over max_edges keys, with a staging of SG_SELECT_MAX_K group edges (a
// longer selection is gathered in pieces through it)
using GroupSelPlan = IndexSelPlan;
inline GroupSelPlan plan_group_select(u64 max_edges, u64 counter_bytes) {
    return plan_index_select(std::max<u64>(max_edges, 1), SG_SELECT_MAX_K, kGrpEdgeBytes, counter_bytes);
}

// K16, the workload rows (sg_group_nodes.h): the device memory sg_set_group_nodes allocates — never sg_create or sg_set_groups.
// Nodes are keyed by K14's group key below GK = max_groups + ncap, at most 2^21: the tables are per key (two of 64 bytes a key and
// the in side's partials: 256 MB + 128 MB at 2^21 keys).  k16_out takes chunks of 2048 group edges; k16_in_part a grid of key ranges
// of 2048 (128 KiB of LDS each) x slices of about 32 K group edges — at most 16 slices, and at most about 1024 workgroups: a
// range's workgroups scan every group edge of their slice, so many ranges take fewer slices, as K11.  k16_count / k16_write follow
// K9's rule over GK.  A window of E group edges has at most min(GK, 2 E) nodes: NC workload rows per slot.
constexpr u64 kGrpNodesMaxKeys = 1ull << 21;
constexpr u32 kGrpNodesMaxInWgs = 1024;
inline int check_group_nodes(u32 max_groups, u32 ncap) { return (u64)max_groups + ncap > kGrpNodesMaxKeys ? SG_EINVAL : SG_OK; }
struct GroupNodesPlan : NodesPlan {
    u64 gk = 0;                   // max_groups + ncap
    u32 max_groups = 0;
    u32 nc = 0;                   // workload rows per window slot: min(GK, 2 x max_edges)
};
inline GroupNodesPlan plan_group_nodes(u64 max_edges, u32 ncap, u32 max_groups, u32 slots) {
    GroupNodesPlan n;
    n.gk = (u64)max_groups + ncap; n.max_groups = max_groups; n.ncap = ncap;
    n.nc = (u32)std::min<u64>(std::max<u64>(n.gk, 1), 2 * std::max<u64>(max_edges, 1));
    plan_rollup(n, max_edges, n.gk, n.nc, kGrpNodesMaxInWgs, slots);
    return n;
}
// K16's baseline: K10's over the workload rows — two samples per row, [NC] sg_node_trend per slot; max_entries defaults to 4 x NC
inline int check_group_node_trend(const sg_trend_params& p, u32 nc, sg_trend_params* out) { return check_node_trend(p, nc, out); }
using GroupNodeTrendPlan = TrendPlan;
inline TrendPlan plan_group_node_trend(u32 nc, u32 slots, const sg_trend_params& p) {
    return plan_baseline(p, 2 * (u64)nc, std::max<u64>(nc, 1) * sizeof(sg_node_trend), slots);
}
// the selection over workload rows: plan_node_select over NC rows
inline NodeSelPlan plan_group_node_select(u32 nc, u64 counter_bytes) { return plan_node_select(nc, counter_bytes); }

// K17, the workload ranking (sg_group_rank.h): the device memory sg_set_group_rank allocates — never sg_create, sg_set_groups or
// sg_set_group_nodes; the parameters are K11's (check_rank).  Work is in ROW-INDEX space: K16's rows are dense, so the per-node
// arrays are [NC] by row position and k17_edge's live ranges are the first ceil(n / 8192) of a window with n rows.
//   range   8192 rows = 64 KiB of u64 accumulators: two 1024-thread workgroups fit a CU's 160 KiB of LDS (K11's 128 KiB range
//           fits one), and a workload window of a few thousand rows is one live range either way
//   slices  one per 2048 group edges, at most 256: the live range of a window with about 590 k group edges and 5.6 k rows then
//           runs 256 workgroups — one per CU — where K11's 32 K rows a slice and 256-workgroup cap give 32.  Each workgroup
//           scans about 2.3 k group edges (under one trip of 1024 threads x 4) and writes min(8192, n) words
//   budget  the partials are [ranges][slices][8192] u64 whether a range is live or not, so slices are cut until they fit in
//           128 MiB (K16's partials at its 2^21-key limit take as much): 256 ranges leave 8 slices, up to 8 ranges all 256
// k17_pos and k17_prep run a grid-stride grid of 256-thread workgroups, at most 1024 (k17_node sums one seed sum per k17_pos
// workgroup); k17_node takes 32 rows a workgroup and round, eight threads sharing the up to 256 partials of a row: a row a thread
// made 22 workgroups of 256 serial loads each on the 5.6 k-row window, 23 us a pass against the edge pass's 9.  The scratch is shared by the window slots; each slot keeps its rank rows; one staging block serves
// sg_window_group_rank's index form and sg_window_group_rank_top.
constexpr u32 kGrpRankThreads = 256, kGrpRankRangeRows = 8192, kGrpRankSliceEdges = 2048, kGrpRankMaxSlices = 256, kGrpRankMaxWgs = 1024,
              kGrpRankNodeRows = 32;
constexpr u64 kGrpRankPartBudget = 128ull << 20;
static_assert(kGrpRankMaxWgs == kRankMaxWgs, "plan_rank_block sizes the seed sums of both rankings");
struct GroupRankPlan : RankBlock {    // (k17_edge, k17_prep over max_edges, k17_node in blocks of 32 rows over nc)
    typedef unsigned long long Weight;   // an element of w (64 bits, as the device code spells them)
    u32 nc = 0;                   // workload rows per window slot (GroupNodesPlan::nc)
    u64 gk = 0;                   // group keys (GroupNodesPlan::gk)
    u32 pos_wgs = 0;              // k17_pos: grid-stride over nc
    u64 pos_bytes = 0;            // [gk] u32 row position by group key
    u64 edge_bytes = 0;           // one per-group-edge u32 array [max_edges] (src, dst: two of them)
    u64 w_bytes = 0;              // [max_edges] u64 weights
    u64 pos_off = 0, edge_off[2] = {}, w_off = 0;   // (edge_off: src, dst)
};
// the workgroups of k17_edge that work on a window of n rows (the others exit at once)
inline u32 group_rank_live_wgs(const GroupRankPlan& r, u64 n) {
    return (u32)std::min<u64>(r.ranges, (n + kGrpRankRangeRows - 1) / kGrpRankRangeRows) * r.slices;
}
inline GroupRankPlan plan_group_rank(u64 max_edges, u32 nc, u64 gk, u32 slots) {
    GroupRankPlan r;
    const u64 ME = std::max<u64>(max_edges, 1), NC = std::max<u32>(nc, 1), GK = std::max<u64>(gk, 1);
    r.nc = nc; r.gk = gk;
    r.ranges = (u32)((NC + kGrpRankRangeRows - 1) / kGrpRankRangeRows);
    r.slices = (u32)std::max<u64>(1, std::min<u64>(kGrpRankMaxSlices, (ME + kGrpRankSliceEdges - 1) / kGrpRankSliceEdges));
    r.slices = (u32)std::max<u64>(1, std::min<u64>(r.slices, kGrpRankPartBudget / ((u64)r.ranges * kGrpRankRangeRows * 8)));
    r.pos_wgs = (u32)std::max<u64>(1, std::min<u64>(kGrpRankMaxWgs, (NC + kGrpRankThreads - 1) / kGrpRankThreads));
    r.prep_wgs = (u32)std::max<u64>(1, std::min<u64>(kGrpRankMaxWgs, (ME + 4 * kGrpRankThreads - 1) / (4 * kGrpRankThreads)));
    r.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kGrpRankMaxWgs, (NC + kGrpRankNodeRows - 1) / kGrpRankNodeRows));
    r.pos_bytes = trend_align(GK * 4);
    r.edge_bytes = trend_align(ME * 4);
    r.w_bytes = trend_align(ME * 8);
    plan_rank_block(r, NC, kGrpRankRangeRows, slots, [&r](Block& b) {
        const char* const edge[2] = {"src", "dst"};
        r.pos_off = b.take("pos", r.pos_bytes);
        for (int k = 0; k < 2; k++) r.edge_off[k] = b.take(edge[k], r.edge_bytes);
        r.w_off = b.take("w", r.w_bytes);
    });
    return r;
}

// K18, the workload incidents (sg_group_incident.h): the device memory sg_set_group_incidents allocates — never sg_create,
// sg_set_groups or sg_set_group_nodes; the parameters are K12's (check_incidents).  Work is in ROW-INDEX space: the row position by
// group key (pos [GK], the stage's own: K17 is optional), four u32 arrays by row position (parent, flag, lab, num), the source
// position of every red group edge (esrc [max_edges]), the max fields' keys by incident and the head counts k9_scan scans are
// scratch shared by the window slots.  k18_label / k18_number take one 256-thread workgroup per block of node_per rows, at most 1024
// blocks (K9's rule); k18_init and k18_finish run a grid-stride grid over NC; k18_hook one over max_edges, at most 1024 workgroups;
// k18_rows at most 256 (K12's reason: every workgroup adds its LDS table to the incidents once); k18_nodes takes kGrpIncFoldRounds
// rounds of 256 rows per workgroup (K13's precedent: fewer workgroups, fewer device atomics on one incident's words, and a
// workgroup can meet more distinct incidents than its table has slots, which then go to device memory directly).  Each slot keeps
// its incident rows, their count and the incident per workload row; one staging block serves sg_window_group_node_incident's index
// form.  Config 3's engine (max_edges 1.25 M, GK = NC = 30 000, two slots): 10.6 MiB in all — 4.8 MiB of esrc, 2 x 2.2 MiB of
// incident rows and node_inc, 0.7 MiB of keys, 0.8 MiB for pos, the four row arrays and the staging.  At K16's limit (2^21 keys,
// max_edges 4 M, two slots) it is 430 MiB, 288 of them the two slots' [NC] incident rows.
constexpr u32 kGrpIncThreads = 256, kGrpIncMaxWgs = 1024, kGrpIncMaxRowWgs = 256, kGrpIncFoldRounds = 8, kGrpIncSlots = 512;
static_assert(kGrpIncThreads == kIncThreads && kGrpIncMaxWgs == kIncMaxWgs && kGrpIncMaxRowWgs == kIncMaxRowWgs,
              "plan_incident_block sizes the grids of both groupings");
struct GroupIncidentPlan : IncidentBlock {
    u32 nc = 0;                   // workload rows per window slot (GroupNodesPlan::nc)
    u64 gk = 0;                   // group keys (GroupNodesPlan::gk)
    u32 fold_wgs = 0;             // k18_nodes: grid-stride over nc, kGrpIncFoldRounds rounds a workgroup
    u64 pos_bytes = 0;            // [gk] u32 row position by group key
    u64 node_bytes = 0;           // one per-row u32 array [nc] (parent, flag, lab, num: four of them)
    u64 esrc_bytes = 0;           // [max_edges] u32
    u64 pos_off = 0, node_off[4] = {}, esrc_off = 0;   // (node_off: parent, flag, lab, num)
};
// the distinct incidents one workgroup of k18_nodes / k18_rows can meet in a window of n workload rows that are all their own
// incident's pair (rows 2i, 2i + 1) / of g group edges each an incident of its own: what the workgroup strides over
inline u64 group_incident_fold_rows(const GroupIncidentPlan& r, u64 n) { return (n + r.fold_wgs - 1) / r.fold_wgs; }
inline u64 group_incident_row_edges(const GroupIncidentPlan& r, u64 g) { return (g + r.row_wgs - 1) / r.row_wgs; }
inline GroupIncidentPlan plan_group_incidents(u64 max_edges, u32 nc, u64 gk, u32 slots) {
    GroupIncidentPlan r;
    const u64 ME = std::max<u64>(max_edges, 1), NC = std::max<u32>(nc, 1), GK = std::max<u64>(gk, 1);
    r.nc = nc; r.gk = gk;
    const u64 fold_rows = (u64)kGrpIncFoldRounds * kGrpIncThreads;
    r.fold_wgs = (u32)std::max<u64>(1, std::min<u64>(kGrpIncMaxWgs, (NC + fold_rows - 1) / fold_rows));
    r.pos_bytes = trend_align(GK * 4);
    r.node_bytes = trend_align(NC * 4);
    r.esrc_bytes = trend_align(ME * 4);
    plan_incident_block(r, max_edges, NC, slots, [&r](Block& b) {
        const char* const node[4] = {"parent", "flag", "lab", "num"};
        r.pos_off = b.take("pos", r.pos_bytes);
        for (int k = 0; k < 4; k++) r.node_off[k] = b.take(node[k], r.node_bytes);
        r.esrc_off = b.take("esrc", r.esrc_bytes);
    });
    return r;
}

// K19, the workload tracks (sg_group_track.h): K13's plan over the workload rows — sg_set_group_tracks allocates it, never
// sg_set_groups, sg_set_group_nodes or sg_set_group_incidents.  The rows, the incident capacity and the ended capacity are K16's nc
// (check_tracks with nc: max_tracks 0 = (quiet_windows + 1) * nc); the members are two u32 arrays by K16's group key below the
// outbound IPs, anchors = max_groups + max_known + max_labels keys, counted in 64 bits: max_groups may reach 2^30, where one array
// alone takes 4 GiB.
inline TrackPlan plan_group_tracks(u32 max_groups, u32 max_known, u32 max_labels, u32 nc, u32 max_tracks, u32 slots) {
    return plan_track_block((u64)max_groups + max_known + max_labels, nc, max_tracks, slots);
}

// K22, the workload impact (sg_group_impact.h): the device memory sg_set_group_impact allocates — never sg_create or any other
// sg_set_* call.  Work is in ROW-INDEX space.  W = ceil(max_incidents / 64) u64 mask words per workload row.  Scratch shared by the
// window slots: the row position by group key (pos [GK], the stage's own), the two round buffers fresh and next ([NC][W] u64 each),
// the call edges' ends ([max_edges] u64), "a call edge arrives here" ([NC] u32), the round counters and the staging of
// sg_window_group_node_hops' index form.  Each slot keeps its mask rows ([NC][W] u64: the search's `have`), its impact rows
// ([max_incidents][8] u64), its hops ([NC] u32) and the covered count.  k22_seed, k22_pull run a grid-stride grid over NC, k22_ends
// and k22_push one over max_edges (4 group edges a thread), each at most 1024 workgroups of 256 threads; k22_finish one over
// max_incidents.  Config 3's engine (max_edges 1.25 M, GK = NC = 30 000, two slots) at the defaults (256 incidents, W = 4): 13.9 MiB
// in all — 9.5 MiB of ends, 2 x 0.9 MiB of fresh / next, 2 x 1.0 MiB of slots; at K16's limit (2^21 keys, max_edges 4 M, two slots)
// with 1024 incidents (W = 16) it is 1.1 GiB, 1 GiB of it the four [NC][16] u64 arrays.
constexpr u32 kImpThreads = 256, kImpMaxWgs = 1024, kImpEdgesPerThread = 4;
inline int check_group_impact(u32 max_incidents, u32 max_hops) {
    return (max_incidents >= 1 && max_incidents <= SG_IMPACT_MAX_INCIDENTS && max_hops >= 1 && max_hops <= SG_IMPACT_MAX_HOPS) ? SG_OK : SG_EINVAL;
}
struct GroupImpactPlan {
    u32 nc = 0;                   // workload rows per window slot (GroupNodesPlan::nc)
    u64 gk = 0;                   // group keys (GroupNodesPlan::gk)
    u32 max_incidents = 0, words = 0;   // words = W
    u32 node_wgs = 0;             // k22_seed, k22_pull: grid-stride over nc
    u32 edge_wgs = 0;             // k22_ends, k22_push: grid-stride over max_edges
    u32 finish_wgs = 0;           // k22_finish: over max_incidents
    u64 pos_bytes = 0;            // [gk] u32
    u64 mask_bytes = 0;           // one [nc][W] u64 array (fresh, next; per slot: mask)
    u64 ends_bytes = 0;           // [max_edges] u64
    u64 node_bytes = 0;           // one [nc] u32 array (arrive, stage, stage_idx; per slot: hops)
    u64 cnt_bytes = 0;            // [SG_IMPACT_MAX_HOPS + 1] u32
    u64 rows_bytes = 0;           // one window slot's impact rows: [max_incidents][8] u64
    u64 count_bytes = 0;          // one window slot's covered count (u64)
    u64 total_bytes = 0;
    u64 pos_off = 0, fresh_off = 0, next_off = 0, ends_off = 0, arrive_off = 0, cnt_off = 0, stage_off = 0, stage_idx_off = 0;
    Slots slot; u64 slot_mask = 0, slot_rows = 0, slot_hops = 0, slot_count = 0;
    std::vector<Piece> layout;
};
inline GroupImpactPlan plan_group_impact(u64 max_edges, u32 nc, u64 gk, u32 slots, u32 max_incidents) {
    GroupImpactPlan r;
    const u64 ME = std::max<u64>(max_edges, 1), NC = std::max<u32>(nc, 1), GK = std::max<u64>(gk, 1), MI = std::max<u32>(max_incidents, 1);
    r.nc = nc; r.gk = gk; r.max_incidents = max_incidents; r.words = (u32)((MI + 63) / 64);
    r.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kImpMaxWgs, (NC + kImpThreads - 1) / kImpThreads));
    const u64 per = (u64)kImpEdgesPerThread * kImpThreads;
    r.edge_wgs = (u32)std::max<u64>(1, std::min<u64>(kImpMaxWgs, (ME + per - 1) / per));
    r.finish_wgs = (u32)((MI + kImpThreads - 1) / kImpThreads);
    r.pos_bytes = trend_align(GK * 4);
    r.mask_bytes = trend_align(NC * r.words * 8);
    r.ends_bytes = trend_align(ME * 8);
    r.node_bytes = trend_align(NC * 4);
    r.cnt_bytes = trend_align(((u64)SG_IMPACT_MAX_HOPS + 1) * 4);
    r.rows_bytes = trend_align(MI * SG_IMPACT_WORDS * 8);
    r.count_bytes = trend_align(8);
    Block b;
    r.pos_off = b.take("pos", r.pos_bytes);
    r.fresh_off = b.take("fresh", r.mask_bytes); r.next_off = b.take("next", r.mask_bytes);
    r.ends_off = b.take("ends", r.ends_bytes);
    r.arrive_off = b.take("arrive", r.node_bytes);
    r.cnt_off = b.take("cnt", r.cnt_bytes);
    r.stage_off = b.take("stage", r.node_bytes); r.stage_idx_off = b.take("stage_idx", r.node_bytes);
    r.slot = b.slots(slots, {{"mask", r.mask_bytes, &r.slot_mask}, {"rows", r.rows_bytes, &r.slot_rows}, {"hops", r.node_bytes, &r.slot_hops},
                             {"count", r.count_bytes, &r.slot_count}});
    r.total_bytes = b.end; r.layout = std::move(b.pieces);
    return r;
}

// K20, the latency percentiles (sg_quantiles.h): the device memory sg_set_quantiles allocates — never sg_create or any other
// sg_set_* call.  One block a space, so that a space goes with its base stage.  Work is in ROW-INDEX space.  Shared by the window slots: the row position by key (pos: [ncap] for the nodes, [gk]
// for the workloads — key spaces, at most 2^21 keys each, K16's rule), one 4-byte target array [max_edges] per side (nodes two,
// group edges one, workloads two) and the partials.  k20_fold runs a grid of ranges of 512 targets (64 KiB of u64 bins in LDS, two
// workgroups a CU) x slices:
//   scattered   (the in sides) every range scans every position of its slice: one slice per 8192 positions, at most 64
//   sorted      (the out sides, the group edges) a range scans its own span only; the slices spread the spans — a few thousand workload
//               rows are a dozen live ranges, and a dozen workgroups would fold a million rows — one per 2048 positions, at most 64
//   budget      a space's partial buffer serves its sides in turn, [ranges][slices][512][16] u64 of the larger side; each side's
//               slices are cut until its partials fit 256 MiB (the group edges of an engine with max_edges 1.25 M: 2442 ranges, one slice)
// Per slot: the histograms (16 u64 an entity and side) and the quantiles (SG_Q_MAX u32 an entity and side) of each space that is
// on.  The group edges' table is 128 + 32 bytes x max_edges a slot: group_slot_bytes reports it, and each space is asked for by
// its own bit because of it.  One staging block of kQStageRows entries serves the index forms of the six reads.
constexpr u32 kQThreads = 256, kQFoldThreads = 512, kQRange = 512, kQMaxWgs = 1024, kQBins = 16, kQMax = 8, kQSliceItems = 8192,
              kQSortedSliceItems = 2048, kQMaxSlices = 64, kQStageRows = 1024;
constexpr u64 kQPartBudget = 256ull << 20, kQMaxKeys = 1ull << 21, kQRangeBytes = (u64)kQRange * kQBins * 8;
static_assert(2 * kQRangeBytes <= kLdsBytes, "two k20_fold workgroups a CU");
// spaces: SG_Q_* bits; the per-mille (n_q == 0: {500, 990}) checked into out[SG_Q_MAX], *n_out of them
inline int check_quantiles(u32 spaces, const u32* permille, u64 n_q, u32 world, u32* out, u32* n_out) {
    if ((spaces & ~(SG_Q_NODES | SG_Q_GROUPS | SG_Q_GROUP_NODES)) || n_q > SG_Q_MAX || world > 1 || (n_q && !permille)) return SG_EINVAL;
    const u32 dflt[2] = {500, 990};
    const u32* p = n_q ? permille : dflt;
    const u32 n = n_q ? (u32)n_q : 2u;
    for (u32 k = 0; k < n; k++) { if (p[k] < 1 || p[k] > 1000) return SG_EINVAL; out[k] = p[k]; }
    *n_out = n;
    return SG_OK;
}
struct QuantSide { u32 ranges = 0, slices = 0; };   // k20_fold's grid of one side: ranges x slices workgroups
struct QuantSpace {
    bool on = false;
    u64 cap = 0;                  // entities per window slot
    u32 sides = 0;                // 2 (out, in) or 1 (group edges)
    QuantSide sorted, scattered;  // the out side / the group edges; the in side
    u32 finish_wgs = 0, pos_wgs = 0, tgt_wgs = 0;
    u64 pos_bytes = 0, pos_off = 0, tgt_off[2] = {};
    u64 part_bytes = 0, part_off = 0;   // [ranges][slices of the larger side][512][16] u64: the sides use it in turn
    u64 stage_off = 0, stage_idx_off = 0;
    u64 hist_bytes = 0, quant_bytes = 0, slot_hist = 0, slot_quant = 0;   // per slot; offsets within the slot
    Slots slot;
    u64 total_bytes = 0;
    std::vector<Piece> layout;
};
struct QuantPlan {
    u32 spaces = 0;
    u64 max_edges = 0;
    QuantSpace sp[3];             // nodes, group edges, workloads: a device block each, freed with its base stage
    u64 tgt_bytes = 0;            // one target array
    u64 group_slot_bytes = 0;     // the group edges' tables per slot (0: the space is off)
    u32 lds_bytes = 0;
    u64 total_bytes = 0;          // of the spaces that are on
};
inline int check_quantile_keys(u32 spaces, u32 ncap, u64 gk) {
    if ((spaces & SG_Q_NODES) && ncap > kQMaxKeys) return SG_EINVAL;
    if ((spaces & SG_Q_GROUP_NODES) && gk > kQMaxKeys) return SG_EINVAL;
    return SG_OK;
}
inline QuantSide plan_quantile_side(u64 cap, u64 max_edges, bool sorted) {
    QuantSide s;
    s.ranges = (u32)((std::max<u64>(cap, 1) + kQRange - 1) / kQRange);
    const u64 per = sorted ? kQSortedSliceItems : kQSliceItems;
    const u64 want = std::min<u64>(kQMaxSlices, (max_edges + per - 1) / per);
    s.slices = (u32)std::max<u64>(1, std::min<u64>(want, kQPartBudget / ((u64)s.ranges * kQRangeBytes)));
    return s;
}
// ncap: the node capacity; gk, nc: K16's group keys and workload rows a slot (read only for SG_Q_GROUP_NODES)
inline QuantPlan plan_quantiles(u64 max_edges, u32 ncap, u64 gk, u32 nc, u32 spaces, u32 slots) {
    QuantPlan q;
    const u64 ME = std::max<u64>(max_edges, 1);
    q.spaces = spaces; q.max_edges = ME;
    q.lds_bytes = (u32)kQRangeBytes;
    q.tgt_bytes = trend_align(ME * 4);
    const u64 caps[3] = {std::max<u32>(ncap, 1), ME, std::max<u32>(nc, 1)}, keys[3] = {std::max<u32>(ncap, 1), 0, std::max<u64>(gk, 1)};
    const char* const tgt_name[2] = {"tgt_out", "tgt_in"};
    for (int k = 0; k < 3; k++) {
        QuantSpace& s = q.sp[k];
        s.on = (spaces >> k) & 1u;
        if (!s.on) continue;
        Block b;
        s.cap = caps[k]; s.sides = k == 1 ? 1 : 2;
        s.sorted = plan_quantile_side(s.cap, ME, true);
        if (s.sides == 2) s.scattered = plan_quantile_side(s.cap, ME, false);
        s.finish_wgs = (u32)std::max<u64>(1, std::min<u64>(kQMaxWgs, (s.cap + kQThreads / kQBins - 1) / (kQThreads / kQBins)));
        s.pos_wgs = (u32)std::max<u64>(1, std::min<u64>(kQMaxWgs, (s.cap + kQThreads - 1) / kQThreads));
        s.tgt_wgs = (u32)std::max<u64>(1, std::min<u64>(kQMaxWgs, (ME + 4 * kQThreads - 1) / (4 * kQThreads)));
        if (keys[k]) { s.pos_bytes = trend_align(keys[k] * 4); s.pos_off = b.take("pos", s.pos_bytes); }
        for (u32 i = 0; i < s.sides; i++) s.tgt_off[i] = b.take(tgt_name[i], q.tgt_bytes);
        s.part_bytes = (u64)s.sorted.ranges * std::max(s.sorted.slices, s.scattered.slices) * kQRangeBytes;
        s.part_off = b.take("part", s.part_bytes);
        s.stage_off = b.take("stage", (u64)kQStageRows * s.sides * kQBins * 8);
        s.stage_idx_off = b.take("stage_idx", (u64)kQStageRows * 4);
        s.hist_bytes = trend_align(s.cap * s.sides * kQBins * 8);
        s.quant_bytes = trend_align(s.cap * s.sides * kQMax * 4);
        s.slot = b.slots(slots, {{"hist", s.hist_bytes, &s.slot_hist}, {"quantiles", s.quant_bytes, &s.slot_quant}});
        s.total_bytes = b.up(b.end); s.layout = std::move(b.pieces);
        q.total_bytes += s.total_bytes;
    }
    q.group_slot_bytes = q.sp[1].on ? q.sp[1].hist_bytes + q.sp[1].quant_bytes : 0;
    return q;
}

// K21, the tail baselines (sg_quantile_trend.h): per requested K20 space the baseline its mean baseline would get — K10's plan over
// the node rows, K15's over the group edges, K16's over the workload rows: the same capacity default, grid, scratch and per-slot
// row table — fed one tracked quantile of K20's table.  sg_set_quantile_trend allocates it, never sg_create or sg_set_quantiles.
// the position of `permille` among the n_q per-mille sg_set_quantiles was last given (the first, if it is there twice), or -1
inline int quantile_index(const u32* qm, u32 n_q, u32 permille) {
    for (u32 k = 0; k < n_q && k < kQMax; k++) if (qm[k] == permille) return (int)k;
    return -1;
}
struct QuantTrendPlan {
    u32 spaces = 0, qi = 0;       // the SG_Q_* bits that are on; the tracked quantile's index
    sg_trend_params params[3] = {};   // the resolved parameters of each space (max_entries defaults differ)
    TrendPlan sp[3];              // nodes, group edges, workloads: a device block each
    u64 total_bytes = 0;          // of the spaces that are on
};
// spaces: the SG_Q_* bits asked for, all of them among `on` (the spaces K20 has on: else SG_ESTATE); qm / n_q: K20's per-mille; ncap,
// max_edges, nc: the capacities the three mean baselines are planned over.  SG_OK and *out, SG_EINVAL or SG_ESTATE
inline int plan_quantile_trend(const sg_trend_params& p, u32 spaces, u32 on, u32 permille, const u32* qm, u32 n_q, u32 ncap, u64 max_edges,
                               u32 nc, u32 slots, QuantTrendPlan* out) {
    if (!spaces || (spaces & ~(SG_Q_NODES | SG_Q_GROUPS | SG_Q_GROUP_NODES))) return SG_EINVAL;
    QuantTrendPlan q;
    if (check_node_trend(p, ncap, &q.params[0]) || check_group_trend(p, max_edges, &q.params[1]) ||
        check_group_node_trend(p, nc, &q.params[2])) return SG_EINVAL;
    const int qi = quantile_index(qm, n_q, permille);
    if (qi < 0) return SG_EINVAL;
    if (spaces & ~on) return SG_ESTATE;
    q.spaces = spaces; q.qi = (u32)qi;
    if (spaces & SG_Q_NODES) q.sp[0] = plan_node_trend(ncap, slots, q.params[0]);
    if (spaces & SG_Q_GROUPS) q.sp[1] = plan_group_trend(max_edges, slots, q.params[1]);
    if (spaces & SG_Q_GROUP_NODES) q.sp[2] = plan_group_node_trend(nc, slots, q.params[2]);
    for (int k = 0; k < 3; k++) q.total_bytes += q.sp[k].total_bytes;
    *out = q;
    return SG_OK;
}

// K23, the traffic baselines (sg_traffic_trend.h): per requested space the baseline its mean baseline gets — K8's plan over the
// window's rows, K10's over the node rows, K15's over the group edges, K16's over the workload rows: the same capacity default,
// grid, scratch and per-slot row table — fed the request count and the busy time.  sg_set_traffic_trend allocates it, never
// sg_create.  The spaces in bit order: 0 edges, 1 nodes, 2 group edges, 3 workloads.
constexpr u32 kTrafficSpaces = 4, kTrafficRateFloor = 8;
constexpr u64 kTrafficLoadFloorNs = 1000000, kTrafficMaxLoadFloorNs = 1ull << 52;
struct TrafficPlan {
    u32 spaces = 0;               // the SG_T_* bits that are on
    double lat_floor = 0, err_floor = 0;   // the floors as the walk gets them: 1000.0 * rate_floor, (double) load_floor_ns
    u32 rate_floor = 0; u64 load_floor_ns = 0;   // resolved
    sg_trend_params params[kTrafficSpaces] = {};   // the resolved walk parameters of each space (max_entries defaults differ; the floors are not these)
    TrendPlan sp[kTrafficSpaces];   // a device block each
    u64 total_bytes = 0;          // of the spaces that are on
};
// spaces: the SG_T_* bits asked for, all of them among `on` (the spaces whose rows are on; the edges always: else SG_ESTATE);
// max_edges, ncap, nc: the capacities the four mean baselines are planned over.  SG_OK and *out, SG_EINVAL or SG_ESTATE
inline int plan_traffic_trend(const sg_traffic_params& p, u32 spaces, u32 on, u64 max_edges, u32 ncap, u32 nc, u32 slots, TrafficPlan* out) {
    if (!spaces || (spaces & ~(SG_T_EDGES | SG_T_NODES | SG_T_GROUPS | SG_T_GROUP_NODES))) return SG_EINVAL;
    if (p.struct_size != sizeof(sg_traffic_params) || p.reserved != 0 || p.load_floor_ns > kTrafficMaxLoadFloorNs) return SG_EINVAL;
    sg_trend_params t{};
    t.struct_size = sizeof(sg_trend_params); t.shift = p.shift; t.warmup = p.warmup; t.ttl = p.ttl; t.max_entries = p.max_entries;
    TrafficPlan q;
    if (check_trend(t, max_edges, &q.params[0]) || check_node_trend(t, ncap, &q.params[1]) || check_group_trend(t, max_edges, &q.params[2]) ||
        check_group_node_trend(t, nc, &q.params[3])) return SG_EINVAL;
    if (spaces & ~on) return SG_ESTATE;
    q.spaces = spaces;
    q.rate_floor = p.rate_floor ? p.rate_floor : kTrafficRateFloor;
    q.load_floor_ns = p.load_floor_ns ? p.load_floor_ns : kTrafficLoadFloorNs;
    q.lat_floor = 1000.0 * (double)q.rate_floor; q.err_floor = (double)q.load_floor_ns;
    if (spaces & SG_T_EDGES) q.sp[0] = plan_trend(max_edges, slots, q.params[0]);
    if (spaces & SG_T_NODES) q.sp[1] = plan_node_trend(ncap, slots, q.params[1]);
    if (spaces & SG_T_GROUPS) q.sp[2] = plan_group_trend(max_edges, slots, q.params[2]);
    if (spaces & SG_T_GROUP_NODES) q.sp[3] = plan_group_node_trend(nc, slots, q.params[3]);
    for (u32 k = 0; k < kTrafficSpaces; k++) q.total_bytes += q.sp[k].total_bytes;
    *out = q;
    return SG_OK;
}

// K24, the SLO burn rates (sg_slo.h): per requested space (SG_Q_NODES: 0, SG_Q_GROUP_NODES: 1) one device block — the ring
// [L][keys][2][3] u64, the sums [keys][2][6] u64, the objective words [keys] u32, the counters, a staging of kSloStageRows rows for the
// index reads and per slot the rows [cap][SG_SLO_WORDS] u64.  keys: the KNOWN and LABEL ids, behind the groups for the workloads;
// at most 2^21.  sg_set_slo allocates it, never sg_create.  At max_known_nodes 15 000, max_labels 64, max_groups 5 564 and L = 64
// the two rings are 46.3 + 63.4 MB: L is the caller's choice for that reason.  Sizes are 64-bit.
constexpr u32 kSloThreads = 256, kSloMaxWgs = 1024, kSloStageRows = 1024, kSloSpaces = 2, kSloCtlWords = 4;
constexpr u64 kSloMaxKeys = 1ull << 21;
struct SloSpace {
    bool on = false;
    u64 keys = 0, cap = 0;        // the key space; the rows a window slot holds
    u32 key_wgs = 0, row_wgs = 0; // k24_retire / k24_count; k24_update
    u64 ring_bytes = 0, sums_bytes = 0, obj_bytes = 0, rows_bytes = 0;
    u64 ring_off = 0, sums_off = 0, obj_off = 0, ctl_off = 0, stage_off = 0, stage_idx_off = 0, slot_rows = 0;
    Slots slot;
    u64 total_bytes = 0;
    std::vector<Piece> layout;
};
struct SloPlan {
    u32 spaces = 0;               // the SG_Q_* bits that are on
    u32 lat_budget = 0, err_budget = 0;   // 10^6 - target, in ppm
    SloSpace sp[kSloSpaces];      // nodes, workloads
    u64 total_bytes = 0;
};
// a budget code of an objective word: exp << 10 | mant -> mant * 10^exp ppm, 0 for a code that is none
inline u32 slo_budget(u32 code) {
    const u32 e = code >> 10 & 3u, m = code & 1023u;
    const u64 b = (u64)m * (e == 0 ? 1u : e == 1 ? 10u : e == 2 ? 100u : 1000u);
    return code >> 12 || m < 1 || m > 1000 || b > 999999 ? 0u : (u32)b;
}
// an objective word sg_slo_assign admits: 0, or a bin of 0 .. 14, bits 27..24 zero and two budget codes
inline bool slo_objective_ok(u32 w) {
    return w == 0 || ((w >> 28) <= 14 && !(w >> 24 & 15u) && slo_budget(w >> 12 & 0xFFFu) && slo_budget(w & 0xFFFu));
}
// spaces: the SG_Q_* bits asked for; on: the spaces K20 has on; mk, ml: max_known_nodes and max_labels; max_groups, nc: K16's (read
// only for SG_Q_GROUP_NODES); ncap: the node rows a slot holds.  SG_OK and *out, SG_EINVAL or SG_ESTATE
inline int plan_slo(const sg_slo_params& p, u32 spaces, u32 on, u64 mk, u64 ml, u64 max_groups, u32 ncap, u32 nc, u32 slots, SloPlan* out) {
    if (!spaces || (spaces & ~(SG_Q_NODES | SG_Q_GROUP_NODES))) return SG_EINVAL;
    if (p.struct_size != sizeof(sg_slo_params) || p.reserved != 0 || p.latency_bin > 14) return SG_EINVAL;
    if (p.latency_target_ppm < 1 || p.latency_target_ppm > 999999 || p.error_target_ppm < 1 || p.error_target_ppm > 999999) return SG_EINVAL;
    if (p.short_windows < 1 || p.short_windows > p.long_windows || p.long_windows > SG_SLO_MAX_WINDOWS) return SG_EINVAL;
    const u64 keys[kSloSpaces] = {mk + ml, max_groups + mk + ml}, caps[kSloSpaces] = {std::max<u32>(ncap, 1), std::max<u32>(nc, 1)};
    const u32 bits[kSloSpaces] = {SG_Q_NODES, SG_Q_GROUP_NODES};
    for (u32 k = 0; k < kSloSpaces; k++) if ((spaces & bits[k]) && keys[k] > kSloMaxKeys) return SG_EINVAL;
    if (spaces & ~on) return SG_ESTATE;
    SloPlan q;
    q.spaces = spaces;
    q.lat_budget = 1000000u - p.latency_target_ppm; q.err_budget = 1000000u - p.error_target_ppm;
    for (u32 k = 0; k < kSloSpaces; k++) {
        SloSpace& s = q.sp[k];
        s.on = (spaces & bits[k]) != 0;
        if (!s.on) continue;
        Block b;
        s.keys = std::max<u64>(keys[k], 1); s.cap = caps[k];
        s.key_wgs = (u32)std::max<u64>(1, std::min<u64>(kSloMaxWgs, (s.keys + kSloThreads - 1) / kSloThreads));
        s.row_wgs = (u32)std::max<u64>(1, std::min<u64>(kSloMaxWgs, (s.cap + kSloThreads - 1) / kSloThreads));
        s.ring_bytes = (u64)p.long_windows * s.keys * 6 * 8; s.sums_bytes = s.keys * 12 * 8; s.obj_bytes = s.keys * 4;
        s.rows_bytes = trend_align(s.cap * SG_SLO_WORDS * 8);
        s.ring_off = b.take("ring", s.ring_bytes);
        s.sums_off = b.take("sums", s.sums_bytes);
        s.obj_off = b.take("objectives", s.obj_bytes);
        s.ctl_off = b.take("ctl", (u64)kSloCtlWords * 8);
        s.stage_off = b.take("stage", (u64)kSloStageRows * SG_SLO_WORDS * 8);
        s.stage_idx_off = b.take("stage_idx", (u64)kSloStageRows * 4);
        s.slot = b.slots(slots, {{"rows", s.rows_bytes, &s.slot_rows}});
        s.total_bytes = b.up(b.end); s.layout = std::move(b.pieces);
        q.total_bytes += s.total_bytes;
    }
    *out = q;
    return SG_OK;
}

// K25, the replica outliers (sg_replicas.h): one device block — the position table pos [gk] u32 (k20_pos_groups' shape), the target
// workload row of every node row tgt [ncap] u32, the member sums' partials [ranges][slices][range_rows][words] u64, the verdicts'
// partials [ranges][slices][range_rows][6] u64, the member sums per workload row [nc][words] u64, a staging of kReplStageRows pod
// rows for the index reads and per slot the pod rows [ncap][12] u32 and the workload rows [nc][8] u32.  words: 4 a side (R, C, E, T),
// and the 16 bins behind them with tails on; range_rows is what 64 KiB of LDS hold of them (1024 or 204 workload rows: two
// k25_fold workgroups a CU); one slice per 2048 node rows, at most 64, cut until the partials fit 256 MiB.  sg_set_replicas
// allocates it, never sg_create.  The parameters come back with their defaults filled in.
constexpr u32 kReplThreads = 256, kReplMaxWgs = 1024, kReplStageRows = 1024, kReplSliceItems = 2048, kReplMaxSlices = 64, kReplSideWords = 4,
              kReplVerdictWords = 6, kReplLdsBytes = 64 * 1024;
constexpr u64 kReplPartBudget = 256ull << 20;
static_assert(2 * kReplLdsBytes <= kLdsBytes, "two k25_fold workgroups a CU");
struct ReplicaPlan {
    bool on = false;
    sg_replica_params p{};        // the parameters in force: no zero left that stands for a default
    u32 tails = 0;                // 1: tail_permille != 0, the stage reads K20's node histograms
    u32 words = 0;                // u64 words a workload row of the member sums: 8, or 40 with tails
    u32 range_rows = 0, ranges = 0, slices = 0;   // k25_fold's grid: ranges x slices workgroups
    u32 lds_bytes = 0, vlds_bytes = 0;            // k25_fold's LDS under the sums' policy and the verdicts'
    u32 node_wgs = 0, group_wgs = 0, sum_wgs = 0, pos_wgs = 0;   // k25_member / k25_rows; k25_groups; k25_reduce; k20_pos_groups
    u64 ncap = 0, nc = 0, gk = 0;
    u64 pos_off = 0, tgt_off = 0, part_off = 0, vpart_off = 0, wsum_off = 0, stage_off = 0, stage_idx_off = 0, slot_pods = 0, slot_groups = 0;
    u64 part_bytes = 0, vpart_bytes = 0, wsum_bytes = 0, pod_bytes = 0, group_bytes = 0;
    Slots slot;
    u64 total_bytes = 0;
    std::vector<Piece> layout;
};
// upstream: bit 0 the node rollup, bit 1 the groups, bit 2 the workload rows, bit 3 K20's SG_Q_NODES space — what is on.  ncap: the
// node rows a slot holds; gk, nc: K16's group keys and workload rows a slot.  SG_OK and *out, SG_EINVAL or SG_ESTATE
inline int plan_replicas(const sg_replica_params& in, u32 world, u32 upstream, u32 ncap, u64 gk, u32 nc, u32 slots, ReplicaPlan* out) {
    if (in.struct_size != sizeof(sg_replica_params) || in.reserved[0] || in.reserved[1] || world > 1) return SG_EINVAL;
    if (in.min_replicas == 1 || in.min_err_excess_q20 > (1u << 20) || in.tail_permille > 999 || in.min_tail_bins > 15) return SG_EINVAL;
    ReplicaPlan q;
    q.p = in;
    if (!q.p.min_replicas) q.p.min_replicas = 3;
    if (!q.p.min_requests) q.p.min_requests = 20;
    if (!q.p.min_err_excess_q20) q.p.min_err_excess_q20 = 20972;
    if (!q.p.min_lat_ratio_q10) q.p.min_lat_ratio_q10 = 2048;
    if (!q.p.min_tail_bins) q.p.min_tail_bins = 2;
    q.tails = q.p.tail_permille != 0;
    if ((upstream & 7u) != 7u || (q.tails && !(upstream & 8u))) return SG_ESTATE;
    if (gk > kQMaxKeys) return SG_EINVAL;
    q.on = true;
    q.ncap = std::max<u32>(ncap, 1); q.nc = std::max<u32>(nc, 1); q.gk = std::max<u64>(gk, 1);
    q.words = 2 * (kReplSideWords + (q.tails ? kQBins : 0u));
    q.range_rows = kReplLdsBytes / (q.words * 8);
    q.ranges = (u32)((q.nc + q.range_rows - 1) / q.range_rows);
    const u64 range_bytes = (u64)q.range_rows * q.words * 8;
    const u64 want = std::min<u64>(kReplMaxSlices, (q.ncap + kReplSliceItems - 1) / kReplSliceItems);
    q.slices = (u32)std::max<u64>(1, std::min<u64>(want, kReplPartBudget / ((u64)q.ranges * range_bytes)));
    q.lds_bytes = (u32)range_bytes; q.vlds_bytes = q.range_rows * kReplVerdictWords * 8;
    q.node_wgs = (u32)std::max<u64>(1, std::min<u64>(kReplMaxWgs, (q.ncap + kReplThreads - 1) / kReplThreads));
    q.group_wgs = (u32)std::max<u64>(1, std::min<u64>(kReplMaxWgs, (q.nc + kReplThreads - 1) / kReplThreads));
    q.sum_wgs = (u32)std::max<u64>(1, std::min<u64>(kReplMaxWgs, (q.nc * q.words + kReplThreads - 1) / kReplThreads));
    q.pos_wgs = (u32)std::max<u64>(1, std::min<u64>(kQMaxWgs, (q.nc + kQThreads - 1) / kQThreads));
    q.part_bytes = (u64)q.ranges * q.slices * range_bytes;
    q.vpart_bytes = (u64)q.ranges * q.slices * q.vlds_bytes;
    q.wsum_bytes = q.nc * q.words * 8;
    q.pod_bytes = trend_align(q.ncap * SG_REPLICA_WORDS * 4); q.group_bytes = trend_align(q.nc * SG_REPLICA_GROUP_WORDS * 4);
    Block b;
    q.pos_off = b.take("pos", trend_align(q.gk * 4));
    q.tgt_off = b.take("tgt", trend_align(q.ncap * 4));
    q.part_off = b.take("part", q.part_bytes);
    q.vpart_off = b.take("vpart", q.vpart_bytes);
    q.wsum_off = b.take("wsum", q.wsum_bytes);
    q.stage_off = b.take("stage", (u64)kReplStageRows * SG_REPLICA_WORDS * 4);
    q.stage_idx_off = b.take("stage_idx", (u64)kReplStageRows * 4);
    q.slot = b.slots(slots, {{"pod_rows", q.pod_bytes, &q.slot_pods}, {"group_rows", q.group_bytes, &q.slot_groups}});
    q.total_bytes = b.up(b.end); q.layout = std::move(b.pieces);
    *out = q;
    return SG_OK;
}

// Does THIS close launch no kc_prepare (Plan::prepare_fold)?  warm: the close keeps the state (not one the back-off closes the plain way);
// warm_try: the host tries the warm path (sg_set_warm), so the close launches the warm attempt; ob_mode 1: the engine collects its own raw
// outbound IPs (0 / 2: a sharded driver's union or gathered lists, which are kc_prepare arguments the attempt's launch does not carry).
inline bool close_folds(const Plan& p, bool warm, bool warm_try, u32 ob_mode) { return p.prepare_fold && warm && warm_try && ob_mode == 1u; }

// the plan's share of the kernels' argument (Dev, sg_device.h; a template so that the CPU test can fill a struct of the same names)
template <class D>
void plan_to_dev(const Plan& p, const sg_config& cfg, D& d) {
    d.max_known = cfg.max_known_nodes; d.max_labels = cfg.max_labels; d.max_obip = p.max_obip;
    d.rank = cfg.rank; d.world = cfg.world; d.max_edges = cfg.max_edges; d.layers = cfg.layers;
    d.ncap = p.ncap; d.emask = p.ecap - 1; d.obmask = p.obcap - 1;
    d.variant = p.variant; d.narrow = p.narrow; d.hist = p.hist; d.agg_slots = p.agg_slots;
    d.nb = p.nb; d.np = p.np; d.pb = p.pb; d.rb = p.rb; d.nwg = p.nwg; d.k1b_split = p.k1b_split; d.npb = p.npb; d.k1b_ht = p.k1b_ht;
    d.pcap = p.pcap; d.sa = p.sa; d.sn = p.sn; d.sw = p.sw; d.punits = p.punits; d.ss = p.ss; d.pslots = p.pslots; d.ovf_cap = p.ovf_cap;
    d.warm = p.warm; d.alive_cap = p.alive_cap; d.hub_cap = p.hub_cap;
    d.k2_sortw = p.k2_sortw; d.dh_g = p.dh_g; d.dh_ppw = p.dh_ppw; d.dh_ns = p.dh_ns;
    d.ablate = p.ablate;
}

}  // namespace sgplan
