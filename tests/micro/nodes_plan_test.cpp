// CPU driver of the node rollup's plan in alaz_amd/csrc/sg_plan.hpp (tests/test_nodes_host.py).  stdin: one "max_edges ncap slots"
// per line; stdout: one JSON object per line — plan_nodes of it and the constants it plans with.
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
        unsigned long long me, ncap, slots;
        in >> me >> ncap >> slots;
        const NodesPlan n = plan_nodes(me, (u32)ncap, (u32)slots);
        std::printf("{\"max_edges\": %llu, \"ncap\": %u, \"slots\": %llu, \"node_size\": %zu, \"out_wgs\": %u, \"ranges\": %u, \"slices\": %u, "
                    "\"node_wgs\": %u, \"node_per\": %u, \"dst_bytes\": %llu, \"table_bytes\": %llu, \"part_bytes\": %llu, \"blk_bytes\": %llu, "
                    "\"rows_bytes\": %llu, \"count_bytes\": %llu, \"lds_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u, \"chunk\": %u, "
                    "\"range_nodes\": %u, \"max_slices\": %u, \"max_wgs\": %u, \"side_bytes\": %llu",
                    me, n.ncap, slots, sizeof(sg_node_out), n.out_wgs, n.ranges, n.slices, n.node_wgs, n.node_per,
                    (unsigned long long)n.dst_bytes, (unsigned long long)n.table_bytes, (unsigned long long)n.part_bytes,
                    (unsigned long long)n.blk_bytes, (unsigned long long)n.rows_bytes, (unsigned long long)n.count_bytes,
                    (unsigned long long)n.lds_bytes, (unsigned long long)n.total_bytes, kNodesThreads, kNodesChunk, kNodesRangeNodes,
                    kNodesMaxSlices, kNodesMaxWgs, (unsigned long long)kNodesSideBytes);
        put_layout("layout", n.layout); put_slot(n.slot, {{"rows", n.slot_rows}, {"count", n.slot_count}});
        std::printf("}\n");
    }
    return 0;
}
