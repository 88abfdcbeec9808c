// CPU driver of the per-edge baselines' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_trend_host.py).  stdin: one
// "max_edges slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved" per line; stdout: one JSON object per
// line (with the block's and one baseline buffer's layout) — check_trend's verdict, the parameters it resolved and plan_trend of them.
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
        unsigned long long me, slots, ss, shift, warmup, ttl, maxe, lf, ef, res;
        in >> me >> slots >> ss >> shift >> warmup >> ttl >> maxe >> lf >> ef >> res;
        sg_trend_params p{(uint32_t)ss, (uint32_t)shift, (uint32_t)warmup, (uint32_t)ttl, maxe, lf, (uint32_t)ef, (uint32_t)res};
        sg_trend_params r{};
        const int rc = check_trend(p, me, &r);
        std::printf("{\"max_edges\": %llu, \"slots\": %llu, \"rc\": %d, \"params_size\": %zu, \"edge_trend_size\": %zu, \"entry_size\": %zu", me, slots, rc,
                    sizeof(sg_trend_params), sizeof(sg_edge_trend), sizeof(sg_trend_entry));
        if (rc == SG_OK) {
            const TrendPlan t = plan_trend(me, (u32)slots, r);
            std::printf(", \"shift\": %u, \"warmup\": %u, \"ttl\": %u, \"max_entries\": %llu, \"lat_floor_ns\": %llu, \"err_floor\": %u, "
                        "\"entries\": %llu, \"wgs\": %u, \"soa_bytes\": %llu, \"ctl_bytes\": %llu, \"blk_bytes\": %llu, \"thread_bytes\": %llu, "
                        "\"rows_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u, \"max_wgs\": %u, \"per_thread\": %u",
                        r.shift, r.warmup, r.ttl, (unsigned long long)r.max_entries, (unsigned long long)r.lat_floor_ns, r.err_floor,
                        (unsigned long long)t.entries, t.wgs, (unsigned long long)t.soa_bytes, (unsigned long long)t.ctl_bytes,
                        (unsigned long long)t.blk_bytes, (unsigned long long)t.thread_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.total_bytes, kTrendThreads, kTrendMaxWgs, kTrendPerThread);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}}); put_layout("soa_layout", t.soa_layout);
        }
        std::printf("}\n");
    }
    return 0;
}
