// CPU driver of the latency percentiles' plan in alaz_amd/csrc/sg_plan.hpp (tests/test_quantile_host.py).  stdin: one
// "max_edges ncap max_groups slots spaces world n_q q0 .. q(n_q - 1)" per line; stdout: one JSON object per line — check_quantiles'
// and check_quantile_keys' verdicts, then plan_quantiles over plan_group_nodes' key count and row capacity: per space its grids,
// sizes, layout and slot region.
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
        unsigned long long me, ncap, mg, slots, spaces, world, nq;
        in >> me >> ncap >> mg >> slots >> spaces >> world >> nq;
        u32 qm[64] = {}, out[SG_Q_MAX] = {}, n_out = 0;
        for (unsigned long long k = 0; k < nq && k < 64; k++) in >> qm[k];
        const GroupNodesPlan n = plan_group_nodes(me, (u32)ncap, (u32)mg, (u32)slots);
        int rc = check_quantiles((u32)spaces, qm, nq, (u32)world, out, &n_out);
        if (rc == SG_OK) rc = check_quantile_keys((u32)spaces, (u32)ncap, n.gk);
        std::printf("{\"max_edges\": %llu, \"ncap\": %llu, \"slots\": %llu, \"spaces\": %llu, \"rc\": %d, \"n_q\": %u, \"permille\": [", me, ncap, slots, spaces, rc, n_out);
        for (u32 k = 0; k < n_out; k++) std::printf("%s%u", k ? ", " : "", out[k]);
        std::printf("]");
        if (rc == SG_OK) {
            const QuantPlan q = plan_quantiles(me, (u32)ncap, n.gk, n.nc, (u32)spaces, (u32)slots);
            std::printf(", \"nc\": %u, \"gk\": %llu, \"tgt_bytes\": %llu, \"group_slot_bytes\": %llu, \"lds_bytes\": %u, \"total_bytes\": %llu, "
                        "\"fold_threads\": %u, \"range\": %u, \"max_wgs\": %u, \"q_max\": %u, \"space\": [",
                        n.nc, (unsigned long long)n.gk, (unsigned long long)q.tgt_bytes, (unsigned long long)q.group_slot_bytes, q.lds_bytes,
                        (unsigned long long)q.total_bytes, kQFoldThreads, kQRange, kQMaxWgs, kQMax);
            for (int k = 0; k < 3; k++) {
                const QuantSpace& s = q.sp[k];
                std::printf("%s{\"on\": %d", k ? ", " : "", s.on ? 1 : 0);
                if (s.on) {
                    std::printf(", \"cap\": %llu, \"sides\": %u, \"sorted\": [%u, %u], \"scattered\": [%u, %u], \"finish_wgs\": %u, \"pos_wgs\": %u, "
                                "\"tgt_wgs\": %u, \"pos_bytes\": %llu, \"part_bytes\": %llu, \"hist_bytes\": %llu, \"quant_bytes\": %llu, \"total_bytes\": %llu",
                                (unsigned long long)s.cap, s.sides, s.sorted.ranges, s.sorted.slices, s.scattered.ranges, s.scattered.slices, s.finish_wgs,
                                s.pos_wgs, s.tgt_wgs, (unsigned long long)s.pos_bytes, (unsigned long long)s.part_bytes, (unsigned long long)s.hist_bytes,
                                (unsigned long long)s.quant_bytes, (unsigned long long)s.total_bytes);
                    put_layout("layout", s.layout); put_slot(s.slot, {{"hist", s.slot_hist}, {"quantiles", s.slot_quant}});
                }
                std::printf("}");
            }
            std::printf("]");
        }
        std::printf("}\n");
    }
    return 0;
}
