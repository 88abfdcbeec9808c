// CPU driver of the culprit ranking's plan in alaz_amd/csrc/sg_plan.hpp (tests/test_rank_host.py).  stdin: one
// "max_edges ncap slots struct_size iters damping_q8 seed reserved" per line; stdout: one JSON object per line — check_rank's verdict,
// the parameters it resolved and plan_rank.
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
        unsigned long long me, nc, slots, ss, iters, damp, seed, res;
        in >> me >> nc >> slots >> ss >> iters >> damp >> seed >> res;
        sg_rank_params p{(uint32_t)ss, (uint32_t)iters, (uint32_t)damp, (uint32_t)seed, 0.0f, (uint32_t)res};
        sg_rank_params r{};
        const int rc = check_rank(p, &r);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"slots\": %llu, \"rc\": %d, \"rank_size\": %zu, \"params_size\": %zu", me, nc, slots, rc,
                    sizeof(sg_node_rank), sizeof(sg_rank_params));
        if (rc == SG_OK) {
            const RankPlan t = plan_rank(me, (u32)nc, (u32)slots);
            std::printf(", \"iters\": %u, \"damping_q8\": %u, \"seed\": %u, \"ranges\": %u, \"slices\": %u, \"prep_wgs\": %u, \"node_wgs\": %u, "
                        "\"row_bytes\": %llu, \"node_bytes\": %llu, \"part_bytes\": %llu, \"seed_bytes\": %llu, \"stage_bytes\": %llu, "
                        "\"stage_idx_bytes\": %llu, \"rows_bytes\": %llu, \"lds_bytes\": %llu, \"total_bytes\": %llu, \"range_nodes\": %u, "
                        "\"max_wgs\": %u, \"max_edge_wgs\": %u, \"lds_limit\": %zu",
                        r.iters, r.damping_q8, r.seed, t.ranges, t.slices, t.prep_wgs, t.node_wgs, (unsigned long long)t.row_bytes,
                        (unsigned long long)t.node_bytes, (unsigned long long)t.part_bytes, (unsigned long long)t.seed_bytes,
                        (unsigned long long)t.stage_bytes, (unsigned long long)t.stage_idx_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.lds_bytes, (unsigned long long)t.total_bytes, kRankRangeNodes, kRankMaxWgs, kRankMaxEdgeWgs, kLdsBytes);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}});
        }
        std::printf("}\n");
    }
    return 0;
}
