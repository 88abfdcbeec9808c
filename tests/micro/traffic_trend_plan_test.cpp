// CPU driver of the traffic baselines' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_traffic_host.py).  stdin: one
// "spaces on max_edges ncap nc slots struct_size shift warmup ttl max_entries load_floor_ns rate_floor reserved" per line; stdout:
// one JSON object per line — plan_traffic_trend's verdict, the resolved floors (as the struct names them and as the walk gets
// them) and, per space that is on, as "sp": [edges, nodes, group edges, workloads] the walk parameters it resolved and the
// baseline's plan (with the block's and one baseline buffer's layout; null for a space that is off).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "plan_layout.hpp"

using namespace sgplan;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        unsigned long long spaces, on, me, ncap, nc, slots, ss, shift, warmup, ttl, maxe, lf, rf, res;
        in >> spaces >> on >> me >> ncap >> nc >> slots >> ss >> shift >> warmup >> ttl >> maxe >> lf >> rf >> res;
        sg_traffic_params p{(uint32_t)ss, (uint32_t)shift, (uint32_t)warmup, (uint32_t)ttl, maxe, lf, (uint32_t)rf, (uint32_t)res};
        TrafficPlan P;
        const int rc = plan_traffic_trend(p, (u32)spaces, (u32)on, me, (u32)ncap, (u32)nc, (u32)slots, &P);
        std::printf("{\"rc\": %d, \"slots\": %llu, \"ncap\": %llu, \"max_edges\": %llu, \"nc\": %llu, \"node_trend_size\": %zu, \"trend_size\": %zu, "
                    "\"params_size\": %zu", rc, slots, ncap, me, nc, sizeof(sg_node_trend), sizeof(sg_edge_trend), sizeof(sg_traffic_params));
        if (rc == SG_OK) {
            std::printf(", \"spaces\": %u, \"rate_floor\": %u, \"load_floor_ns\": %llu, \"lat_floor\": %.17g, \"err_floor\": %.17g, \"total_bytes\": %llu, \"sp\": [",
                        P.spaces, P.rate_floor, (unsigned long long)P.load_floor_ns, P.lat_floor, P.err_floor, (unsigned long long)P.total_bytes);
            for (u32 k = 0; k < kTrafficSpaces; k++) {
                if (k) std::printf(", ");
                if (!((P.spaces >> k) & 1u)) { std::printf("null"); continue; }
                const TrendPlan& t = P.sp[k];
                const sg_trend_params& r = P.params[k];
                std::printf("{\"slots\": %llu, \"shift\": %u, \"warmup\": %u, \"ttl\": %u, \"max_entries\": %llu, "
                            "\"entries\": %llu, \"wgs\": %u, \"soa_bytes\": %llu, \"ctl_bytes\": %llu, \"blk_bytes\": %llu, \"thread_bytes\": %llu, "
                            "\"rows_bytes\": %llu, \"total_bytes\": %llu, \"per_thread\": %u",
                            slots, r.shift, r.warmup, r.ttl, (unsigned long long)r.max_entries,
                            (unsigned long long)t.entries, t.wgs, (unsigned long long)t.soa_bytes, (unsigned long long)t.ctl_bytes,
                            (unsigned long long)t.blk_bytes, (unsigned long long)t.thread_bytes, (unsigned long long)t.rows_bytes,
                            (unsigned long long)t.total_bytes, kTrendPerThread);
                put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}}); put_layout("soa_layout", t.soa_layout);
                std::printf("}");
            }
            std::printf("]");
        }
        std::printf("}\n");
    }
    return 0;
}
