// CPU driver of the selection plan in alaz_amd/csrc/sg_plan.hpp (tests/test_select_host.py).  stdin: one max_edges per line;
// stdout: one JSON object per line — plan_select(max_edges, used = true / false) and k7_sort's LDS at SG_SELECT_MAX_K.
#include <cstdio>
#include <iostream>
#include <string>

#include "../../alaz_amd/csrc/sg_plan.hpp"

using namespace sgplan;

static void put(const char* name, const SelPlan& s) {
    std::printf("\"%s\": {\"wgs\": %u, \"key_bytes\": %llu, \"hist_bytes\": %llu, \"blk_bytes\": %llu, \"pair_bytes\": %llu, \"state_bytes\": %llu, "
                "\"scratch_bytes\": %llu, \"stage_rows\": %llu}", name, s.wgs, (unsigned long long)s.key_bytes, (unsigned long long)s.hist_bytes,
                (unsigned long long)s.blk_bytes, (unsigned long long)s.pair_bytes, (unsigned long long)s.state_bytes,
                (unsigned long long)s.scratch_bytes, (unsigned long long)s.stage_rows);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const u64 me = std::stoull(line);
        std::printf("{\"max_edges\": %llu, ", (unsigned long long)me);
        put("used", plan_select(me, true)); std::printf(", ");
        put("unused", plan_select(me, false));
        std::printf(", \"sort_lds_max_k\": %zu, \"sort_lds_1\": %zu, \"lds_bytes\": %zu, \"max_k\": %u, \"threads\": %u, \"max_wgs\": %u, \"rows_per_wg\": %u}\n",
                    select_sort_lds(SG_SELECT_MAX_K), select_sort_lds(1), kLdsBytes, (unsigned)SG_SELECT_MAX_K, kSelThreads, kSelMaxWgs, kSelRowsPerWg);
    }
    return 0;
}
