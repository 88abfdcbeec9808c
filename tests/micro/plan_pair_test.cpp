// plan_pair_test.cpp — pass A's tile pairs in the plan (sg_plan.hpp: PassA::k1a_pair, PassAKernel::pair), on the CPU.
//
//   g++ -O2 -std=c++17 -o plan_pair_test tests/micro/plan_pair_test.cpp
//
// One case per input line, `name key=value ...` — sg_config members by name, the development build's SG_* knobs and l1= / l2=, the
// join tables' level-1 entries and level-2 bytes (default: the tables as sg_create builds them), as plan_test.cpp takes them.  One
// JSON object per case: what the LDS layout of k1a_team_partition is made of, pass A's choice and the kernel key it leads to.
// --domains: the team kernel's instantiations, without and with pairs.
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

template <size_t N, size_t M>
static std::string keys_json(const char* name, const std::array<Key<N>, M>& keys) {
    std::ostringstream o;
    o << '"' << name << "\": [";
    for (size_t i = 0; i < M; i++) { o << (i ? ", [" : "["); for (size_t k = 0; k < N; k++) o << (k ? ", " : "") << keys[i][k]; o << "]"; }
    o << "]";
    return o.str();
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--domains")) {
        std::cout << "{" << keys_json("k1a_team", kK1aTeamKeys) << ", " << keys_json("k1a_team_pair", kK1aTeamPairKeys) << "}" << std::endl;
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string name, tok; is >> name;
        sg_config c; std::memset(&c, 0, sizeof c);
        c.struct_size = sizeof c; c.abi_version = SG_ABI_VERSION; c.layers = 2; c.world = 1; c.max_outbound_ips = 64; c.max_labels = 64;
        DeviceFacts dev;
        Overrides ov;
        u64 l1 = 0, l2 = 0; bool given = false;
        while (is >> tok) {
            const size_t eq = tok.find('='); const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            const u64 x = std::strtoull(v.c_str(), nullptr, 0);
            bool known = false;
            for (const KnobName& kn : kKnobs) if (k == kn.name) { ov.*kn.field = v; known = true; }
            if (known) continue;
            if (k == "max_known_nodes") c.max_known_nodes = (u32)x; else if (k == "max_labels") c.max_labels = (u32)x;
            else if (k == "max_outbound_ips") c.max_outbound_ips = (u32)x; else if (k == "max_ips") c.max_ips = (u32)x;
            else if (k == "max_edges") c.max_edges = x; else if (k == "layers") c.layers = (u32)x;
            else if (k == "rank") c.rank = (u32)x; else if (k == "world") c.world = (u32)x; else if (k == "k1_variant") c.k1_variant = (u32)x;
            else if (k == "max_window_events") c.max_window_events = x; else if (k == "flags") c.flags = (u32)x;
            else if (k == "l1") { l1 = x; given = true; } else if (k == "l2") { l2 = x; given = true; }
            else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
        }
        sg_config cfg; Plan p; std::string why;
        int rc = check_config(c, &cfg);
        if (rc == SG_OK) rc = make_plan(cfg, dev, ov, &p, &why);
        PassA pa;
        if (rc == SG_OK) {
            if (!given) {
                sgjoin::Table jt; std::vector<u32> mirror;
                const sgjoin::Layout L = sgjoin::Table::make_layout(cfg.max_ips, cfg.max_known_nodes, p.max_blocks);
                mirror.assign(L.words, 0);
                jt.init(L, mirror.data(), p.variant == 0);
                l1 = jt.l1_entries; l2 = jt.blocks_bytes();
            }
            if (p.variant != 0 || !plan_pass_a(p, (u32)l1, (size_t)l2, ov, &pa)) rc = SG_ENOSPC;
        }
        std::ostringstream o;
        o << "{\"name\": \"" << name << "\", \"rc\": " << rc;
        if (rc == SG_OK) {
            const PassAKernel k = choose_pass_a(p, pa, cfg);
            o << ", \"np\": " << p.np << ", \"nb\": " << p.nb << ", \"narrow\": " << p.narrow << ", \"l1_entries\": " << l1 << ", \"l2_bytes\": " << l2
              << ", \"l2_u16\": " << pa.l2_u16 << ", \"l2_in_lds\": " << pa.l2_in_lds << ", \"k1a_team\": " << pa.k1a_team << ", \"k1a_teams\": " << pa.k1a_teams
              << ", \"k1a_nt\": " << pa.k1a_nt << ", \"k1a_ct\": " << pa.k1a_ct << ", \"k1a_lds\": " << pa.k1a_lds << ", \"k1a_pair\": " << pa.k1a_pair
              << ", \"k1a_pair_lds\": " << pa.k1a_pair_lds << ", \"lds_cap\": " << kLdsBytes << ", \"pair_default\": " << kK1aPairDefault
              << ", \"kernel\": {\"family\": " << k.family << ", \"l2\": " << k.l2 << ", \"sharded\": " << k.sharded << ", \"pb\": " << k.pb
              << ", \"pair\": " << k.pair << "}";
        }
        o << "}";
        std::cout << o.str() << std::endl;
    }
    return 0;
}
