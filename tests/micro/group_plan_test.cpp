// CPU driver of the groups' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_group_host.py).  stdin: one
// "max_edges max_known ncap max_groups slots world struct_size reserved0 reserved1" per line; stdout: one JSON object per line —
// check_groups' verdict and plan_groups.
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
        unsigned long long me, mk, nc, mg, slots, world, ss, r0, r1;
        in >> me >> mk >> nc >> mg >> slots >> world >> ss >> r0 >> r1;
        sg_group_params p{(uint32_t)ss, (uint32_t)mg, {(uint32_t)r0, (uint32_t)r1}};
        sg_group_params r{};
        const int rc = check_groups(p, (u32)mk, (u32)world, &r);
        std::printf("{\"max_edges\": %llu, \"max_known\": %llu, \"ncap\": %llu, \"slots\": %llu, \"rc\": %d, \"edge_size\": %zu, \"params_size\": %zu", me, mk, nc,
                    slots, rc, sizeof(sg_group_edge), sizeof(sg_group_params));
        if (rc == SG_OK) {
            const GroupPlan t = plan_groups(me, (u32)mk, (u32)nc, r.max_groups, (u32)slots);
            std::printf(", \"max_groups\": %u, \"gk\": %llu, \"kb\": %u, \"key_bytes\": %u, \"passes\": %u, \"tiles\": %u, \"key_wgs\": %u, \"chunks\": %u, "
                        "\"cpw\": %u, \"heads_wgs\": %u, \"stitch_wgs\": %u, \"keys_bytes\": %llu, \"idx_bytes\": %llu, \"map_bytes\": %llu, "
                        "\"hist_bytes\": %llu, \"chunkcnt_bytes\": %llu, \"part_bytes\": %llu, \"meta_bytes\": %llu, \"blk_bytes\": %llu, "
                        "\"stage_bytes\": %llu, \"rows_bytes\": %llu, \"count_bytes\": %llu, \"total_bytes\": %llu, \"tile\": %u, \"chunk\": %u, \"max_wgs\": %u",
                        t.max_groups, (unsigned long long)t.gk, t.kb, t.key_bytes, t.passes, t.tiles, t.key_wgs, t.chunks, t.cpw, t.heads_wgs, t.stitch_wgs,
                        (unsigned long long)t.keys_bytes, (unsigned long long)t.idx_bytes, (unsigned long long)t.map_bytes, (unsigned long long)t.hist_bytes,
                        (unsigned long long)t.chunkcnt_bytes, (unsigned long long)t.part_bytes, (unsigned long long)t.meta_bytes,
                        (unsigned long long)t.blk_bytes, (unsigned long long)t.stage_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.count_bytes, (unsigned long long)t.total_bytes, kGrpTile, kGrpChunk, kGrpMaxWgs);
            put_layout("layout", t.layout);
            put_slot(t.slot, {{"rows", t.slot_rows}, {"count", t.slot_count}, {"row_group", t.slot_row_group}, {"perm", t.slot_perm}});
        }
        std::printf("}\n");
    }
    return 0;
}
