// CPU driver of the vanished list's plan in alaz_amd/csrc/sg_plan.hpp (tests/test_vanish_host.py).  stdin: one
// "max_edges slots warmup ttl max_entries struct_size silent_windows min_seen max_rows" per line; stdout: one JSON object per line —
// check_vanished's verdict against the trend those parameters resolve to, the parameters it resolved and plan_vanished of them.
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
        unsigned long long me, slots, warmup, ttl, maxe, ss, silent, seen, rows;
        in >> me >> slots >> warmup >> ttl >> maxe >> ss >> silent >> seen >> rows;
        sg_trend_params tp{(uint32_t)sizeof(sg_trend_params), 0, (uint32_t)warmup, (uint32_t)ttl, maxe, 0, 0, 0};
        sg_trend_params tr{};
        if (check_trend(tp, me, &tr) != SG_OK) { std::printf("{\"trend_rc\": -1}\n"); continue; }
        const TrendPlan t = plan_trend(me, (u32)slots, tr);
        sg_vanished_params p{(uint32_t)ss, (uint32_t)silent, (uint32_t)seen, (uint32_t)rows};
        sg_vanished_params r{};
        const int rc = check_vanished(p, tr, &r);
        std::printf("{\"max_edges\": %llu, \"slots\": %llu, \"rc\": %d, \"params_size\": %zu, \"vanished_size\": %zu, \"ttl\": %u, "
                    "\"warmup\": %u, \"entries\": %llu, \"wgs\": %u", me, slots, rc, sizeof(sg_vanished_params), sizeof(sg_edge_vanished),
                    tr.ttl, tr.warmup, (unsigned long long)t.entries, t.wgs);
        if (rc == SG_OK) {
            const VanishedPlan v = plan_vanished(t, (u32)slots, r);
            std::printf(", \"silent_windows\": %u, \"min_seen\": %u, \"max_rows\": %u, \"rows\": %llu, \"thread_bytes\": %llu, \"blk_bytes\": %llu, "
                        "\"list_bytes\": %llu, \"count_bytes\": %llu, \"total_bytes\": %llu, \"threads\": %u",
                        r.silent_windows, r.min_seen, r.max_rows, (unsigned long long)v.rows, (unsigned long long)v.thread_bytes,
                        (unsigned long long)v.blk_bytes, (unsigned long long)v.list_bytes, (unsigned long long)v.count_bytes,
                        (unsigned long long)v.total_bytes, kTrendThreads);
            put_layout("layout", v.layout); put_slot(v.slot, {{"list", v.slot_list}, {"count", v.slot_count}});
        }
        std::printf("}\n");
    }
    return 0;
}
