// CPU driver of the workload baselines' plans in alaz_amd/csrc/sg_plan.hpp (tests/test_group_trend_host.py).  stdin: one
// "max_edges slots struct_size shift warmup ttl max_entries lat_floor_ns err_floor reserved vstruct_size silent_windows min_seen
// max_rows counter_bytes" per line; stdout: one JSON object per line — check_group_trend's verdict, the parameters it resolved and
// plan_group_trend of them (with the block's and one baseline buffer's layout); as "van" check_vanished's verdict against them and
// plan_vanished over that plan; as "sel" plan_group_select(max_edges, counter_bytes).
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
        unsigned long long me, slots, ss, shift, warmup, ttl, maxe, lf, ef, res, vss, silent, seen, rows, cb;
        in >> me >> slots >> ss >> shift >> warmup >> ttl >> maxe >> lf >> ef >> res >> vss >> silent >> seen >> rows >> cb;
        sg_trend_params p{(uint32_t)ss, (uint32_t)shift, (uint32_t)warmup, (uint32_t)ttl, maxe, lf, (uint32_t)ef, (uint32_t)res};
        sg_trend_params r{};
        const int rc = check_group_trend(p, me, &r);
        std::printf("{\"max_edges\": %llu, \"slots\": %llu, \"rc\": %d, \"trend_size\": %zu, \"group_edge_size\": %zu", me, slots, rc,
                    sizeof(sg_edge_trend), sizeof(sg_group_edge));
        if (rc == SG_OK) {
            const GroupTrendPlan t = plan_group_trend(me, (u32)slots, r);
            std::printf(", \"shift\": %u, \"warmup\": %u, \"ttl\": %u, \"max_entries\": %llu, \"lat_floor_ns\": %llu, \"err_floor\": %u, "
                        "\"entries\": %llu, \"wgs\": %u, \"soa_bytes\": %llu, \"ctl_bytes\": %llu, \"blk_bytes\": %llu, \"thread_bytes\": %llu, "
                        "\"rows_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u, \"max_wgs\": %u, \"per_thread\": %u",
                        r.shift, r.warmup, r.ttl, (unsigned long long)r.max_entries, (unsigned long long)r.lat_floor_ns, r.err_floor,
                        (unsigned long long)t.entries, t.wgs, (unsigned long long)t.soa_bytes, (unsigned long long)t.ctl_bytes,
                        (unsigned long long)t.blk_bytes, (unsigned long long)t.thread_bytes, (unsigned long long)t.rows_bytes,
                        (unsigned long long)t.total_bytes, kTrendThreads, kTrendMaxWgs, kTrendPerThread);
            put_layout("layout", t.layout); put_slot(t.slot, {{"rows", t.slot_rows}}); put_layout("soa_layout", t.soa_layout);
            sg_vanished_params vp{(uint32_t)vss, (uint32_t)silent, (uint32_t)seen, (uint32_t)rows};
            sg_vanished_params vr{};
            const int vrc = check_vanished(vp, r, &vr);
            std::printf(", \"van\": {\"rc\": %d, \"slots\": %llu", vrc, slots);
            if (vrc == SG_OK) {
                const VanishedPlan v = plan_vanished(t, (u32)slots, vr);
                std::printf(", \"silent_windows\": %u, \"min_seen\": %u, \"max_rows\": %u, \"rows\": %llu, \"total_bytes\": %llu",
                            vr.silent_windows, vr.min_seen, vr.max_rows, (unsigned long long)v.rows, (unsigned long long)v.total_bytes);
                put_layout("layout", v.layout); put_slot(v.slot, {{"list", v.slot_list}, {"count", v.slot_count}});
            }
            std::printf("}");
        }
        const GroupSelPlan g = plan_group_select(me, cb);
        std::printf(", \"sel\": {\"slots\": 1, \"wgs\": %u, \"stage_rows\": %llu, \"scratch_bytes\": %llu, \"key_bytes\": %llu, \"total_bytes\": %llu, "
                    "\"select_max_k\": %u", g.sel.wgs, (unsigned long long)g.stage_rows, (unsigned long long)g.sel.scratch_bytes,
                    (unsigned long long)g.sel.key_bytes, (unsigned long long)g.total_bytes, SG_SELECT_MAX_K);
        put_layout("layout", g.layout); put_layout("k7_layout", g.sel.layout);
        std::printf("}}\n");
    }
    return 0;
}
