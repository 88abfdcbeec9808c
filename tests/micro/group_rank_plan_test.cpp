// CPU driver of the workload ranking's plan in alaz_amd/csrc/sg_plan.hpp (tests/test_group_rank_host.py).  stdin: one
// "max_edges ncap max_groups slots rows struct_size iters damping_q8 seed reserved" per line; stdout: one JSON object per line —
// check_rank's verdict, the parameters it resolved, plan_group_rank over plan_group_nodes' row capacity and key count, and the
// workgroups of k17_edge that work on a window of `rows` workload rows.
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
        unsigned long long me, ncap, mg, slots, rows, ss, iters, damp, seed, res;
        in >> me >> ncap >> mg >> slots >> rows >> ss >> iters >> damp >> seed >> res;
        sg_rank_params p{(uint32_t)ss, (uint32_t)iters, (uint32_t)damp, (uint32_t)seed, 0.0f, (uint32_t)res};
        sg_rank_params r{};
        const int rc = check_rank(p, &r);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"max_groups\": %llu, \"slots\": %llu, \"rc\": %d, \"rank_size\": %zu, \"params_size\": %zu",
                    me, ncap, mg, slots, rc, sizeof(sg_node_rank), sizeof(sg_rank_params));
        if (rc == SG_OK) {
            const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
            const GroupRankPlan t = plan_group_rank(me, n.nc, n.gk, (u32)slots);
            std::printf(", \"iters\": %u, \"damping_q8\": %u, \"seed\": %u, \"nc\": %u, \"gk\": %llu, \"ranges\": %u, \"slices\": %u, \"pos_wgs\": %u, "
                        "\"prep_wgs\": %u, \"node_wgs\": %u, \"pos_bytes\": %llu, \"edge_bytes\": %llu, \"w_bytes\": %llu, \"node_bytes\": %llu, "
                        "\"part_bytes\": %llu, \"seed_bytes\": %llu, \"stage_bytes\": %llu, \"stage_idx_bytes\": %llu, \"rows_bytes\": %llu, "
                        "\"lds_bytes\": %llu, \"total_bytes\": %llu, \"range_rows\": %u, \"slice_edges\": %u, \"max_slices\": %u, \"max_wgs\": %u, "
                        "\"part_budget\": %llu, \"lds_limit\": %zu, \"live_wgs\": %u",
                        r.iters, r.damping_q8, r.seed, t.nc, (unsigned long long)t.gk, t.ranges, t.slices, t.pos_wgs, t.prep_wgs, t.node_wgs,
                        (unsigned long long)t.pos_bytes, (unsigned long long)t.edge_bytes, (unsigned long long)t.w_bytes,
                        (unsigned long long)t.node_bytes, (unsigned long long)t.part_bytes, (unsigned long long)t.seed_bytes,
                        (unsigned long long)t.stage_bytes, (unsigned long long)t.stage_idx_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.lds_bytes, (unsigned long long)t.total_bytes, kGrpRankRangeRows, kGrpRankSliceEdges,
                        kGrpRankMaxSlices, kGrpRankMaxWgs, (unsigned long long)kGrpRankPartBudget, kLdsBytes, group_rank_live_wgs(t, rows));
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}});
        }
        std::printf("}\n");
    }
    return 0;
}
