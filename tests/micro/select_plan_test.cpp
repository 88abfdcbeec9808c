// CPU driver of the selection plan in alaz_amd/csrc/sg_plan.hpp (tests/test_select_host.py).  stdin: one max_edges per line;
// stdout: one JSON object per line — plan_select(max_edges, used = true / false), the scratch's layout, the node selection's block
// over max_edges node rows with a counter block of kCtrBytes (plan_node_select) and k7_sort's LDS at SG_SELECT_MAX_K.
#include <cstdio>
#include <iostream>
#include <string>

#include "plan_layout.hpp"

using namespace sgplan;

constexpr u64 kCtrBytes = 200;            // any size that is no multiple of 256: the engine passes its own counter block's

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
        put_layout("layout", plan_select(me, true).layout);
        const NodeSelPlan n = plan_node_select((u32)me, kCtrBytes);
        std::printf(", \"node\": {\"ctr_in\": %llu, \"sel_scratch_bytes\": %llu, \"sel_off\": %llu, \"total_bytes\": %llu",
                    (unsigned long long)kCtrBytes, (unsigned long long)n.sel.scratch_bytes, (unsigned long long)n.sel_off, (unsigned long long)n.total_bytes);
        put_layout("layout", n.layout); put_layout("sel_layout", n.sel.layout);
        std::printf("}");
        std::printf(", \"sort_lds_max_k\": %zu, \"sort_lds_1\": %zu, \"lds_bytes\": %zu, \"max_k\": %u, \"threads\": %u, \"max_wgs\": %u, \"rows_per_wg\": %u}\n",
                    select_sort_lds(SG_SELECT_MAX_K), select_sort_lds(1), kLdsBytes, (unsigned)SG_SELECT_MAX_K, kSelThreads, kSelMaxWgs, kSelRowsPerWg);
    }
    return 0;
}
