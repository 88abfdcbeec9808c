// CPU driver of the workload impact's plan in alaz_amd/csrc/sg_plan.hpp (tests/test_group_impact_host.py).  stdin: one
// "max_edges ncap max_groups slots max_incidents max_hops" per line; stdout: one JSON object per line — check_group_impact's verdict
// and plan_group_impact over plan_group_nodes' row capacity and key count.
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
        unsigned long long me, ncap, mg, slots, mi, mh;
        in >> me >> ncap >> mg >> slots >> mi >> mh;
        const int rc = (mi > 0xFFFFFFFFull || mh > 0xFFFFFFFFull) ? SG_EINVAL : check_group_impact((u32)mi, (u32)mh);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"max_groups\": %llu, \"slots\": %llu, \"max_incidents\": %llu, \"max_hops\": %llu, \"rc\": %d, "
                    "\"impact_words\": %u, \"limit_incidents\": %u, \"limit_hops\": %u",
                    me, ncap, mg, slots, mi, mh, rc, SG_IMPACT_WORDS, SG_IMPACT_MAX_INCIDENTS, SG_IMPACT_MAX_HOPS);
        if (rc == SG_OK) {
            const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
            const GroupImpactPlan t = plan_group_impact(me, n.nc, n.gk, (u32)slots, (u32)mi);
            std::printf(", \"nc\": %u, \"gk\": %llu, \"words\": %u, \"node_wgs\": %u, \"edge_wgs\": %u, \"finish_wgs\": %u, \"launches\": %llu, "
                        "\"pos_bytes\": %llu, \"mask_bytes\": %llu, \"ends_bytes\": %llu, \"node_bytes\": %llu, \"cnt_bytes\": %llu, \"rows_bytes\": %llu, "
                        "\"count_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u, \"max_wgs\": %u",
                        t.nc, (unsigned long long)t.gk, t.words, t.node_wgs, t.edge_wgs, t.finish_wgs, 2 * mh + 4, (unsigned long long)t.pos_bytes,
                        (unsigned long long)t.mask_bytes, (unsigned long long)t.ends_bytes, (unsigned long long)t.node_bytes,
                        (unsigned long long)t.cnt_bytes, (unsigned long long)t.rows_bytes, (unsigned long long)t.count_bytes,
                        (unsigned long long)t.total_bytes, kImpThreads, kImpMaxWgs);
            put_layout("layout", t.layout);
            put_slot(t.slot, {{"mask", t.slot_mask}, {"rows", t.slot_rows}, {"hops", t.slot_hops}, {"count", t.slot_count}});
        }
        std::printf("}\n");
    }
    return 0;
}
