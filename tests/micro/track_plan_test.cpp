// CPU driver of the tracks' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_track_host.py).  stdin: one
// "max_known max_labels ncap slots struct_size quiet_windows max_tracks reserved" per line; stdout: one JSON object per line —
// check_tracks' verdict and plan_tracks.
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
        unsigned long long mk, ml, nc, slots, ss, quiet, mt, res;
        in >> mk >> ml >> nc >> slots >> ss >> quiet >> mt >> res;
        sg_track_params p{(uint32_t)ss, (uint32_t)quiet, (uint32_t)mt, (uint32_t)res};
        sg_track_params r{};
        const int rc = check_tracks(p, (u32)nc, &r);
        std::printf("{\"max_known\": %llu, \"max_labels\": %llu, \"ncap\": %llu, \"slots\": %llu, \"rc\": %d, \"row_size\": %zu, \"entry_size\": %zu, "
                    "\"params_size\": %zu, \"stats_size\": %zu",
                    mk, ml, nc, slots, rc, sizeof(sg_incident_track), sizeof(sg_track_entry), sizeof(sg_track_params), sizeof(sg_track_stats));
        if (rc == SG_OK) {
            const TrackPlan t = plan_tracks((u32)mk, (u32)ml, (u32)nc, r.max_tracks, (u32)slots);
            std::printf(", \"quiet\": %u, \"max_tracks\": %u, \"anchors\": %u, \"wgs\": %u, \"per\": %u, \"init_wgs\": %u, \"node_wgs\": %u, \"fold_wgs\": %u, \"fold_rounds\": %u, "
                        "\"member_bytes\": %llu, \"table_bytes\": %llu, \"state_bytes\": %llu, \"inc_bytes\": %llu, \"claim_bytes\": %llu, "
                        "\"blk_bytes\": %llu, \"rows_bytes\": %llu, \"ended_bytes\": %llu, \"count_bytes\": %llu, \"total_bytes\": %llu, "
                        "\"threads\": %u, \"max_wgs\": %u",
                        r.quiet_windows, t.max_tracks, t.anchors, t.wgs, t.per, t.init_wgs, t.node_wgs, t.fold_wgs, kTrkFoldRounds, (unsigned long long)t.member_bytes,
                        (unsigned long long)t.table_bytes, (unsigned long long)t.state_bytes, (unsigned long long)t.inc_bytes,
                        (unsigned long long)t.claim_bytes, (unsigned long long)t.blk_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.ended_bytes, (unsigned long long)t.count_bytes, (unsigned long long)t.total_bytes, kTrkThreads,
                        kTrkMaxWgs);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}, {"ended", t.slot_ended}, {"ended_count", t.slot_count}});
        }
        std::printf("}\n");
    }
    return 0;
}
