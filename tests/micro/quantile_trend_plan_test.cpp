// CPU driver of the tail baselines' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_quantile_trend_host.py).  stdin: one
// "spaces on permille n_q q0 .. q7 ncap max_edges nc slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved"
// per line; stdout: one JSON object per line — plan_quantile_trend's verdict, the tracked index and, per space that is on, as
// "sp": [nodes, group edges, workloads] the parameters it resolved and the baseline's plan (with the block's and one baseline
// buffer's layout; null for a space that is off).
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
        unsigned long long spaces, on, permille, nq, q[8], ncap, me, nc, slots, ss, shift, warmup, ttl, maxe, lf, ef, res;
        in >> spaces >> on >> permille >> nq;
        for (int k = 0; k < 8; k++) in >> q[k];
        in >> ncap >> me >> nc >> slots >> ss >> shift >> warmup >> ttl >> maxe >> lf >> ef >> res;
        u32 qm[8];
        for (int k = 0; k < 8; k++) qm[k] = (u32)q[k];
        sg_trend_params p{(uint32_t)ss, (uint32_t)shift, (uint32_t)warmup, (uint32_t)ttl, maxe, lf, (uint32_t)ef, (uint32_t)res};
        QuantTrendPlan P;
        const int rc = plan_quantile_trend(p, (u32)spaces, (u32)on, (u32)permille, qm, (u32)nq, (u32)ncap, me, (u32)nc, (u32)slots, &P);
        std::printf("{\"rc\": %d, \"slots\": %llu, \"ncap\": %llu, \"max_edges\": %llu, \"nc\": %llu, \"node_trend_size\": %zu, \"trend_size\": %zu",
                    rc, slots, ncap, me, nc, sizeof(sg_node_trend), sizeof(sg_edge_trend));
        if (rc == SG_OK) {
            std::printf(", \"spaces\": %u, \"qi\": %u, \"total_bytes\": %llu, \"sp\": [", P.spaces, P.qi, (unsigned long long)P.total_bytes);
            for (int k = 0; k < 3; k++) {
                if (k) std::printf(", ");
                if (!((P.spaces >> k) & 1u)) { std::printf("null"); continue; }
                const TrendPlan& t = P.sp[k];
                const sg_trend_params& r = P.params[k];
                std::printf("{\"slots\": %llu, \"shift\": %u, \"warmup\": %u, \"ttl\": %u, \"max_entries\": %llu, \"lat_floor_ns\": %llu, \"err_floor\": %u, "
                            "\"entries\": %llu, \"wgs\": %u, \"soa_bytes\": %llu, \"ctl_bytes\": %llu, \"blk_bytes\": %llu, \"thread_bytes\": %llu, "
                            "\"rows_bytes\": %llu, \"total_bytes\": %llu, \"per_thread\": %u",
                            slots, r.shift, r.warmup, r.ttl, (unsigned long long)r.max_entries, (unsigned long long)r.lat_floor_ns, r.err_floor,
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
