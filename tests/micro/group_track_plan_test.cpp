// CPU driver of the workload tracks' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_group_track_host.py).  stdin: one
// "max_groups max_known max_labels nc slots struct_size quiet_windows max_tracks reserved" per line; stdout: one JSON object per
// line — check_tracks' verdict over nc and plan_group_tracks.
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
        unsigned long long mg, mk, ml, nc, slots, ss, quiet, mt, res;
        in >> mg >> mk >> ml >> nc >> slots >> ss >> quiet >> mt >> res;
        sg_track_params p{(uint32_t)ss, (uint32_t)quiet, (uint32_t)mt, (uint32_t)res};
        sg_track_params r{};
        const int rc = check_tracks(p, (u32)nc, &r);
        std::printf("{\"max_groups\": %llu, \"max_known\": %llu, \"max_labels\": %llu, \"nc\": %llu, \"slots\": %llu, \"rc\": %d", mg, mk, ml, nc, slots, rc);
        if (rc == SG_OK) {
            const TrackPlan t = plan_group_tracks((u32)mg, (u32)mk, (u32)ml, (u32)nc, r.max_tracks, (u32)slots);
            std::printf(", \"quiet\": %u, \"max_tracks\": %u, \"ncap\": %u, \"anchors\": %u, \"wgs\": %u, \"per\": %u, \"init_wgs\": %u, \"node_wgs\": %u, \"fold_wgs\": %u, "
                        "\"member_bytes\": %llu, \"table_bytes\": %llu, \"state_bytes\": %llu, \"inc_bytes\": %llu, \"claim_bytes\": %llu, "
                        "\"blk_bytes\": %llu, \"rows_bytes\": %llu, \"ended_bytes\": %llu, \"count_bytes\": %llu, \"total_bytes\": %llu",
                        r.quiet_windows, t.max_tracks, t.ncap, t.anchors, t.wgs, t.per, t.init_wgs, t.node_wgs, t.fold_wgs, (unsigned long long)t.member_bytes,
                        (unsigned long long)t.table_bytes, (unsigned long long)t.state_bytes, (unsigned long long)t.inc_bytes,
                        (unsigned long long)t.claim_bytes, (unsigned long long)t.blk_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.ended_bytes, (unsigned long long)t.count_bytes, (unsigned long long)t.total_bytes);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}, {"ended", t.slot_ended}, {"ended_count", t.slot_count}});
        }
        std::printf("}\n");
    }
    return 0;
}
