// plan_k3_forms_test.cpp — K3's two batched-load forms in the plan (sg_plan.hpp: Plan::k3_in_form / k3_feat_lanes, Kernels likewise,
// SG_K3_IN_FORM / SG_K3_FEAT_LANES), on the CPU.
//
//   g++ -O2 -std=c++17 -o plan_k3_forms_test tests/micro/plan_k3_forms_test.cpp
//
// One case per input line, `name key=value ...` — sg_config members by name, the development build's SG_* knobs and cus= (compute
// units), as plan_test.cpp takes them.  One JSON object per case: make_plan's return code and message, the two forms as the plan and
// the kernel choice have them, what they hang on (k5_form, k5_efeat, the slices) and the defaults.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../alaz_amd/csrc/join_host.hpp"
#include "../../alaz_amd/csrc/sg_plan.hpp"

using namespace sgplan;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string name, tok; is >> name;
        sg_config c; std::memset(&c, 0, sizeof c);
        c.struct_size = sizeof c; c.abi_version = SG_ABI_VERSION; c.layers = 2; c.world = 1; c.max_outbound_ips = 64; c.max_labels = 64;
        DeviceFacts dev;
        Overrides ov;
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
            else if (k == "cus") dev.cus = (int)x;
            else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
        }
        sg_config cfg; Plan p; std::string why;
        int rc = check_config(c, &cfg);
        if (rc == SG_OK) rc = make_plan(cfg, dev, ov, &p, &why);
        std::ostringstream o;
        o << "{\"name\": \"" << name << "\", \"rc\": " << rc << ", \"why\": \"" << why << "\"";
        if (rc == SG_OK) {
            PassA pa;
            const Kernels k = choose_kernels(p, pa, cfg);
            o << ", \"k3_in_form\": " << p.k3_in_form << ", \"k3_feat_lanes\": " << p.k3_feat_lanes << ", \"kernel_in_form\": " << k.k3_in_form
              << ", \"kernel_feat_lanes\": " << k.k3_feat_lanes << ", \"k5_form\": " << p.k5_form << ", \"k5_efeat\": " << p.k5_efeat
              << ", \"k3_slices\": " << p.k3_slices << ", \"k3_ranges\": " << p.k3_ranges << ", \"in_form_default\": " << k3_in_form_default(cfg)
              << ", \"in_form_on\": " << (kK3InFormDefault ? 1 : 0) << ", \"feat_lanes_on\": " << (kK3FeatLanesDefault ? 1 : 0);
        }
        o << "}";
        std::cout << o.str() << std::endl;
    }
    return 0;
}
