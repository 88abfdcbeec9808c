// CPU driver of the workload incidents' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_group_incident_host.py).  stdin: one
// "max_edges ncap max_groups slots rows group_edges struct_size by reserved" per line; stdout: one JSON object per line —
// check_incidents' verdict, plan_group_incidents over plan_group_nodes' row capacity and key count, and what one workgroup of each
// folding pass strides over in a window of `rows` workload rows and `group_edges` group edges.
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
        unsigned long long me, ncap, mg, slots, rows, ge, ss, by, res;
        in >> me >> ncap >> mg >> slots >> rows >> ge >> ss >> by >> res;
        sg_incident_params p{(uint32_t)ss, (uint32_t)by, 0.5f, (uint32_t)res};
        sg_incident_params r{};
        const int rc = check_incidents(p, &r);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"max_groups\": %llu, \"slots\": %llu, \"rc\": %d, \"out_size\": %zu, \"params_size\": %zu",
                    me, ncap, mg, slots, rc, sizeof(sg_incident_out), sizeof(sg_incident_params));
        if (rc == SG_OK) {
            const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
            const GroupIncidentPlan t = plan_group_incidents(me, n.nc, n.gk, (u32)slots);
            std::printf(", \"by\": %u, \"nc\": %u, \"gk\": %llu, \"node_wgs\": %u, \"node_per\": %u, \"grid_wgs\": %u, \"fold_wgs\": %u, \"hook_wgs\": %u, "
                        "\"row_wgs\": %u, \"pos_bytes\": %llu, \"node_bytes\": %llu, \"esrc_bytes\": %llu, \"keys_bytes\": %llu, \"blk_bytes\": %llu, "
                        "\"stage_bytes\": %llu, \"rows_bytes\": %llu, \"count_bytes\": %llu, \"node_inc_bytes\": %llu, \"total_bytes\": %llu, "
                        "\"threads\": %u, \"max_wgs\": %u, \"max_row_wgs\": %u, \"fold_rounds\": %u, \"table_slots\": %u, \"fold_rows\": %llu, "
                        "\"row_edges\": %llu",
                        r.by, t.nc, (unsigned long long)t.gk, t.node_wgs, t.node_per, t.grid_wgs, t.fold_wgs, t.hook_wgs, t.row_wgs,
                        (unsigned long long)t.pos_bytes, (unsigned long long)t.node_bytes, (unsigned long long)t.esrc_bytes,
                        (unsigned long long)t.keys_bytes, (unsigned long long)t.blk_bytes, (unsigned long long)t.stage_bytes,
                        (unsigned long long)t.rows_bytes, (unsigned long long)t.count_bytes, (unsigned long long)t.node_inc_bytes,
                        (unsigned long long)t.total_bytes, kGrpIncThreads, kGrpIncMaxWgs, kGrpIncMaxRowWgs, kGrpIncFoldRounds, kGrpIncSlots,
                        (unsigned long long)group_incident_fold_rows(t, rows), (unsigned long long)group_incident_row_edges(t, ge));
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"node_inc", t.slot_node_inc}});
        }
        std::printf("}\n");
    }
    return 0;
}
