// CPU driver of alaz_amd/csrc/sg_plan.hpp (tests/test_plan.py).  stdin: one case per line,
//   name key=value ...   config fields (sg_config names), SG_* overrides, l1= / l2= join-table sizes for a second pass-A plan.
// stdout: one JSON object per case — the plan, the Dev fields the engine fills from it at create, pass A for the join tables as
// sg_create builds them and, given l1 / l2, pass A for those sizes; "kernels" (and "kernels_after") is the kernel instantiation each
// launch site takes under that plan.  --knobs: the knob names, one per line.  --domains: the instantiations the library holds, per
// kernel family, as lists of template arguments (one JSON object).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../alaz_amd/csrc/join_host.hpp"
#include "../../alaz_amd/csrc/sg_plan.hpp"

using namespace sgplan;

// Dev's scalar fields (alaz_amd/csrc/sg_device.h), zero as at create
struct DevScalars {
    u32 ipmask, ipmask2, jl1mask, jl2_words, ck_n, jstage_bytes, jl2_in_lds, max_known, max_labels, max_obip, rank, world, emask, obmask;
    u64 max_edges;
    u32 variant, np, nwg, ss, sa, pslots, k1a_ct, narrow, nb, pb, rb, k1b_split, npb, sn, sw, punits, k1b_ht, hist, agg_slots, ovf_cap, pcap,
        batch_state, ablate, k2_sortw, k1a_rot, k1a_ticket_base, alive_cap, warm, kept_compact, dh_g, dh_ppw, dh_ns, hub_cap, ncap, layers;
};

struct Json {
    std::ostringstream o; bool first = true;
    void kv(const char* k, unsigned long long v) { o << (first ? "" : ", ") << '"' << k << "\": " << v; first = false; }
    std::string str() const { return "{" + o.str() + "}"; }
};

static std::string pass_a_json(u32 l1, size_t l2, const PassA& a) {
    Json j;
    j.kv("l1_entries", l1); j.kv("l2_bytes", l2); j.kv("l2_u16", a.l2_u16); j.kv("k1a_nsub", a.k1a_nsub); j.kv("k1a_team", a.k1a_team);
    j.kv("k1a_teams", a.k1a_teams); j.kv("k1a_nt", a.k1a_nt); j.kv("k1a_ct", a.k1a_ct); j.kv("l2_in_lds", a.l2_in_lds); j.kv("k1a_lds", a.k1a_lds);
    return j.str();
}

static std::string kernels_json(const Kernels& k) {
    Json j;
    j.kv("k1a_family", k.k1a.family); j.kv("k1a_l2", k.k1a.l2); j.kv("k1a_sharded", k.k1a.sharded); j.kv("k1a_hist", k.k1a.hist);
    j.kv("k1a_nsub", k.k1a.nsub); j.kv("k1a_pb", k.k1a.pb);
    j.kv("k1b_family", k.k1b_family); j.kv("k1b_u", k.k1b_u); j.kv("k1b_spt", k.k1b_spt); j.kv("k1b_pack", k.k1b_pack); j.kv("k1b_hist", k.k1b_hist);
    j.kv("k1b_share", k.k1b_share); j.kv("k1b_warm", k.k1b_warm);
    j.kv("k2_dh", k.k2_dh); j.kv("k4_split", k.k4_split); j.kv("k4_mfma", k.k4_mfma); j.kv("k5_mfma", k.k5_mfma);
    return j.str();
}

template <size_t N, size_t M>
static std::string keys_json(const char* name, const std::array<Key<N>, M>& keys) {
    std::ostringstream o;
    o << '"' << name << "\": [";
    for (size_t i = 0; i < M; i++) { o << (i ? ", [" : "["); for (size_t k = 0; k < N; k++) o << (k ? ", " : "") << keys[i][k]; o << "]"; }
    o << "]";
    return o.str();
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--knobs")) { for (const KnobName& k : kKnobs) std::printf("%s\n", k.name); return 0; }
    if (argc > 1 && !std::strcmp(argv[1], "--domains")) {
        std::cout << "{" << keys_json("k1a_wide", kK1aWideKeys) << ", " << keys_json("k1a_tile", kK1aTileKeys) << ", " << keys_json("k1a_team", kK1aTeamKeys)
                  << ", " << keys_json("k1b_merge", kK1bMergeKeys) << ", " << keys_json("k1b_stream", kK1bStreamKeys) << ", " << keys_json("k4_layer", kK4LayerKeys)
                  << ", \"k1b_warm_u\": " << kK1bWarmU << "}" << std::endl;
        return 0;
    }
    DeviceFacts dev;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string name, tok; is >> name;
        sg_config c; std::memset(&c, 0, sizeof c);
        c.struct_size = sizeof c; c.abi_version = SG_ABI_VERSION; c.layers = 2; c.world = 1; c.max_outbound_ips = 64; c.max_labels = 64;
        Overrides ov;
        u64 l1 = 0, l2 = 0; bool after = false;
        while (is >> tok) {
            const size_t eq = tok.find('='); const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            const u64 x = std::strtoull(v.c_str(), nullptr, 0);
            bool known = false;
            for (const KnobName& kn : kKnobs) if (k == kn.name) { ov.*kn.field = v; known = true; }
            if (known) continue;
            if (k == "max_known_nodes") c.max_known_nodes = (u32)x; else if (k == "max_labels") c.max_labels = (u32)x;
            else if (k == "max_outbound_ips") c.max_outbound_ips = (u32)x; else if (k == "max_ips") c.max_ips = (u32)x;
            else if (k == "max_edges") c.max_edges = x; else if (k == "max_batch") c.max_batch = (u32)x; else if (k == "layers") c.layers = (u32)x;
            else if (k == "rank") c.rank = (u32)x; else if (k == "world") c.world = (u32)x; else if (k == "k1_variant") c.k1_variant = (u32)x;
            else if (k == "max_window_events") c.max_window_events = x; else if (k == "windows_in_flight") c.windows_in_flight = (u32)x;
            else if (k == "max_alive") c.max_alive = (u32)x; else if (k == "flags") c.flags = (u32)x;
            else if (k == "cus") dev.cus = (int)x;
            else if (k == "l1") { l1 = x; after = true; } else if (k == "l2") { l2 = x; after = true; }
            else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
        }
        std::ostringstream o;
        o << "{\"name\": \"" << name << "\"";
        sg_config cfg; Plan p; std::string why;
        int rc = check_config(c, &cfg);
        if (rc == SG_OK) rc = make_plan(cfg, dev, ov, &p, &why);
        // the join tables as sg_create builds them: pass A is planned for their initial state
        PassA pa; sgjoin::Table jt; std::vector<u32> mirror; sgjoin::Layout L{};
        if (rc == SG_OK) {
            L = sgjoin::Table::make_layout(cfg.max_ips, cfg.max_known_nodes, p.max_blocks);
            mirror.assign(L.words, 0);
            jt.init(L, mirror.data(), p.variant == 0);
            if (p.variant == 0 && !plan_pass_a(p, jt.l1_entries, jt.blocks_bytes(), ov, &pa)) rc = SG_ENOSPC;
        }
        o << ", \"rc\": " << rc;
        if (rc == SG_OK) {
            DevScalars d{};
            plan_to_dev(p, cfg, d);
            d.ipmask = L.ipcap - 1; d.ipmask2 = L.ip2cap - 1;
            Json j;
#define P(x) j.kv(#x, (u64)p.x)
#define D(x) j.kv(#x, (u64)d.x)
            D(variant); D(narrow); D(hist); D(agg_slots); D(nb); D(np); D(pb); D(nwg); D(k1b_split); D(k1b_ht); D(npb); D(rb); D(pcap); D(sa); D(sn); D(sw);
            D(punits); D(ss); D(pslots); D(ovf_cap); D(warm); P(k1b_threads); P(k1b_u); P(k1b_pack); P(k1b_lds);
            P(ecap); P(obcap); P(ob_list_cap); D(ncap); D(alive_cap); D(hub_cap); P(max_blocks);
            P(k3_ranges); P(k3_slices); P(k3in_lds); D(k2_sortw); D(dh_g); D(dh_ppw); D(dh_ns);
            P(k4_split); P(k5_grid); P(k3_fuse_allowed); P(k6_one_wg); P(use_mfma);
            P(k1b_order); P(k1_grid); P(n_copy); P(n_stage); P(arena_on); P(n_slots); D(ablate);
            D(ipmask); D(ipmask2); D(jl1mask); D(jl2_words); D(ck_n); D(jstage_bytes); D(jl2_in_lds); D(max_known); D(max_labels); D(max_obip);
            D(rank); D(world); D(emask); D(obmask); D(max_edges); D(k1a_ct); D(batch_state); D(k1a_rot); D(k1a_ticket_base); D(kept_compact); D(layers);
#undef P
#undef D
            o << ", \"cus\": " << p.cus << ", \"plan\": " << j.str() << ", \"pass_a\": " << pass_a_json(jt.l1_entries, jt.blocks_bytes(), pa);
            Kernels kn = choose_kernels(p, pa, cfg);
            o << ", \"kernels\": " << kernels_json(kn);
            if (after) {
                PassA pb = pa;                                      // (the engine keeps its geometry when the tables leave no legal one)
                const bool ok = p.variant != 0 || plan_pass_a(p, (u32)l1, (size_t)l2, ov, &pb);
                o << ", \"upsert_rc\": " << (ok ? SG_OK : SG_ENOSPC) << ", \"pass_a_after\": " << pass_a_json((u32)l1, (size_t)l2, pb);
                kn.k1a = choose_pass_a(p, pb, cfg);                // (the rest of the choice is made once, at create)
                o << ", \"kernels_after\": " << kernels_json(kn);
            }
        }
        o << "}";
        std::cout << o.str() << std::endl;
    }
    return 0;
}
