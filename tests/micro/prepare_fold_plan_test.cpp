// prepare_fold_plan_test.cpp — which window closes launch no kc_prepare (sg_plan.hpp: Plan::prepare_fold, close_folds), on the CPU.
//
//   g++ -O2 -std=c++17 -o prepare_fold_plan_test tests/micro/prepare_fold_plan_test.cpp
//
// One case per input line, `name key=value ...` — sg_config members by name, cus, and the development build's SG_* knobs, as
// plan_test.cpp takes them.  One JSON object per case: the plan's choice, the facts it rests on, and close_folds for every
// (the close keeps state, the host tries the warm path, outbound-IP mode) a close can come with.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

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
            else if (k == "max_edges") c.max_edges = x; else if (k == "layers") c.layers = (u32)x;
            else if (k == "rank") c.rank = (u32)x; else if (k == "world") c.world = (u32)x; else if (k == "k1_variant") c.k1_variant = (u32)x;
            else if (k == "max_window_events") c.max_window_events = x; else if (k == "windows_in_flight") c.windows_in_flight = (u32)x;
            else if (k == "flags") c.flags = (u32)x; else if (k == "cus") dev.cus = (int)x;
            else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
        }
        sg_config cfg; Plan p; std::string why;
        int rc = check_config(c, &cfg);
        if (rc == SG_OK) rc = make_plan(cfg, dev, ov, &p, &why);
        std::ostringstream o;
        o << "{\"name\": \"" << name << "\", \"rc\": " << rc;
        if (rc == SG_OK) {
            o << ", \"prepare_fold\": " << (p.prepare_fold ? 1 : 0) << ", \"warm\": " << p.warm << ", \"narrow\": " << p.narrow << ", \"variant\": " << p.variant
              << ", \"k1b_threads\": " << p.k1b_threads << ", \"k1b_lds\": " << p.k1b_lds << ", \"prepare_lds\": " << kPrepareLds << ", \"closes\": [";
            bool first = true;
            for (int warm = 0; warm < 2; warm++) for (int wt = 0; wt < 2; wt++) for (u32 ob = 0; ob < 3; ob++) {
                o << (first ? "" : ", ") << "[" << warm << ", " << wt << ", " << ob << ", " << (close_folds(p, warm != 0, wt != 0, ob) ? 1 : 0) << "]";
                first = false;
            }
            o << "]";
        }
        o << "}";
        std::cout << o.str() << std::endl;
    }
    return 0;
}
