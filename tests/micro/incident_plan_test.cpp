// CPU driver of the incidents' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_incident_host.py).  stdin: one
// "max_edges ncap slots struct_size by reserved" per line; stdout: one JSON object per line — check_incidents' verdict and
// plan_incidents.
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
        unsigned long long me, nc, slots, ss, by, res;
        in >> me >> nc >> slots >> ss >> by >> res;
        sg_incident_params p{(uint32_t)ss, (uint32_t)by, 0.5f, (uint32_t)res};
        sg_incident_params r{};
        const int rc = check_incidents(p, &r);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"slots\": %llu, \"rc\": %d, \"out_size\": %zu, \"params_size\": %zu", me, nc, slots, rc,
                    sizeof(sg_incident_out), sizeof(sg_incident_params));
        if (rc == SG_OK) {
            const IncidentPlan t = plan_incidents(me, (u32)nc, (u32)slots);
            std::printf(", \"by\": %u, \"min_value\": %g, \"node_wgs\": %u, \"node_per\": %u, \"grid_wgs\": %u, \"hook_wgs\": %u, \"row_wgs\": %u, "
                        "\"key_bytes\": %llu, \"keys_bytes\": %llu, \"blk_bytes\": %llu, \"stage_bytes\": %llu, \"rows_bytes\": %llu, "
                        "\"count_bytes\": %llu, \"node_inc_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u, \"max_wgs\": %u, \"max_row_wgs\": %u",
                        r.by, (double)r.min_value, t.node_wgs, t.node_per, t.grid_wgs, t.hook_wgs, t.row_wgs, (unsigned long long)t.key_bytes,
                        (unsigned long long)t.keys_bytes, (unsigned long long)t.blk_bytes, (unsigned long long)t.stage_bytes,
                        (unsigned long long)t.rows_bytes, (unsigned long long)t.count_bytes, (unsigned long long)t.node_inc_bytes,
                        (unsigned long long)t.total_bytes, kIncThreads, kIncMaxWgs, kIncMaxRowWgs);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"node_inc", t.slot_node_inc}});
        }
        std::printf("}\n");
    }
    return 0;
}
