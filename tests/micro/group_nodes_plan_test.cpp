// CPU driver of the workload rows' plans in alaz_amd/csrc/sg_plan.hpp (tests/test_group_nodes_host.py).  stdin: one
// "max_edges ncap max_groups slots max_entries counter_bytes" per line; stdout: one JSON object per line — check_group_nodes'
// verdict and plan_group_nodes (with the block's layout); as "trend" check_group_node_trend's verdict over default parameters with
// that max_entries and plan_group_node_trend; as "sel" plan_group_node_select(NC, counter_bytes).
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
        unsigned long long me, ncap, mg, slots, maxe, cb;
        in >> me >> ncap >> mg >> slots >> maxe >> cb;
        const int rc = check_group_nodes((u32)mg, (u32)ncap);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"max_groups\": %llu, \"slots\": %llu, \"rc\": %d, \"node_size\": %zu, \"node_trend_size\": %zu",
                    me, ncap, mg, slots, rc, sizeof(sg_node_out), sizeof(sg_node_trend));
        if (rc == SG_OK) {
            const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
            std::printf(", \"gk\": %llu, \"nc\": %u, \"out_wgs\": %u, \"ranges\": %u, \"slices\": %u, \"node_wgs\": %u, \"node_per\": %u, "
                        "\"dst_bytes\": %llu, \"table_bytes\": %llu, \"part_bytes\": %llu, \"blk_bytes\": %llu, \"rows_bytes\": %llu, "
                        "\"count_bytes\": %llu, \"lds_bytes\": %llu, \"total_bytes\": %llu, \"max_wgs\": %u, \"lds_limit\": %zu",
                        (unsigned long long)n.gk, n.nc, n.out_wgs, n.ranges, n.slices, n.node_wgs, n.node_per, (unsigned long long)n.dst_bytes,
                        (unsigned long long)n.table_bytes, (unsigned long long)n.part_bytes, (unsigned long long)n.blk_bytes,
                        (unsigned long long)n.rows_bytes, (unsigned long long)n.count_bytes, (unsigned long long)n.lds_bytes,
                        (unsigned long long)n.total_bytes, kNodesMaxWgs, kLdsBytes);
            put_layout("layout", n.layout); put_slot(n.slot, {{"rows", n.slot_rows}, {"count", n.slot_count}});
            sg_trend_params p{};
            p.struct_size = sizeof(sg_trend_params); p.max_entries = maxe;
            sg_trend_params r{};
            const int trc = check_group_node_trend(p, n.nc, &r);
            std::printf(", \"trend\": {\"rc\": %d, \"slots\": %llu", trc, slots);
            if (trc == SG_OK) {
                const GroupNodeTrendPlan t = plan_group_node_trend(n.nc, (u32)slots, r);
                std::printf(", \"max_entries\": %llu, \"entries\": %llu, \"wgs\": %u, \"soa_bytes\": %llu, \"rows_bytes\": %llu, \"total_bytes\": %llu, "
                            "\"per_thread\": %u",
                            (unsigned long long)r.max_entries, (unsigned long long)t.entries, t.wgs, (unsigned long long)t.soa_bytes,
                            (unsigned long long)t.rows_bytes, (unsigned long long)t.total_bytes, kTrendPerThread);
                put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}}); put_layout("soa_layout", t.soa_layout);
            }
            std::printf("}");
            const NodeSelPlan g = plan_group_node_select(n.nc, cb);
            std::printf(", \"sel\": {\"slots\": 1, \"wgs\": %u, \"scratch_bytes\": %llu, \"key_bytes\": %llu, \"total_bytes\": %llu", g.sel.wgs,
                        (unsigned long long)g.sel.scratch_bytes, (unsigned long long)g.sel.key_bytes, (unsigned long long)g.total_bytes);
            put_layout("layout", g.layout); put_layout("k7_layout", g.sel.layout);
            std::printf("}");
        }
        std::printf("}\n");
    }
    return 0;
}
