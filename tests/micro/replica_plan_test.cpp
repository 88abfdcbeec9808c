// The CPU driver of plan_replicas (alaz_amd/csrc/sg_plan.hpp) for tests/test_replicas_host.py: one JSON object per input line.
//   replica_plan_test  "world upstream ncap gk nc slots struct_size min_replicas min_requests min_err_excess_q20 min_lat_ratio_q10
//                       tail_permille min_tail_bins reserved0 reserved1": plan_replicas' verdict, the parameters in force, the
//                       fold's grid and LDS, the other grids and the block's layout
#include <iostream>

#include "plan_json.hpp"

using namespace sgplan;
typedef unsigned long long ull;

static int plan_line(const std::string& line) {
    std::istringstream is(line);
    ull v[15] = {};
    for (ull& x : v) if (!(is >> x)) { std::fprintf(stderr, "replica_plan_test: 15 numbers a line: %s\n", line.c_str()); return 2; }
    sg_replica_params p{};
    p.struct_size = (u32)v[6]; p.min_replicas = (u32)v[7]; p.min_requests = v[8]; p.min_err_excess_q20 = (u32)v[9]; p.min_lat_ratio_q10 = (u32)v[10];
    p.tail_permille = (u32)v[11]; p.min_tail_bins = (u32)v[12]; p.reserved[0] = (u32)v[13]; p.reserved[1] = (u32)v[14];
    ReplicaPlan P;
    const int rc = plan_replicas(p, (u32)v[0], (u32)v[1], (u32)v[2], v[3], (u32)v[4], (u32)v[5], &P);
    Json j;
    j.kv("rc", rc).kv("slots", v[5]).kv("params_size", sizeof(sg_replica_params)).kv("row_words", SG_REPLICA_WORDS);
    j.kv("group_row_words", SG_REPLICA_GROUP_WORDS).kv("stage_rows", kReplStageRows).kv("lds_budget", kReplLdsBytes);
    if (rc == SG_OK) {
        j.obj("params");
        PUT(P.p, min_replicas); PUT(P.p, min_requests); PUT(P.p, min_err_excess_q20); PUT(P.p, min_lat_ratio_q10); PUT(P.p, tail_permille);
        PUT(P.p, min_tail_bins);
        j.end();
        PUT(P, tails); PUT(P, words); PUT(P, range_rows); PUT(P, ranges); PUT(P, slices); PUT(P, lds_bytes); PUT(P, vlds_bytes);
        PUT(P, node_wgs); PUT(P, group_wgs); PUT(P, sum_wgs); PUT(P, pos_wgs); PUT(P, ncap); PUT(P, nc); PUT(P, gk);
        PUT(P, part_bytes); PUT(P, vpart_bytes); PUT(P, wsum_bytes); PUT(P, pod_bytes); PUT(P, group_bytes);
        PUT(P, pos_off); PUT(P, tgt_off); PUT(P, part_off); PUT(P, vpart_off); PUT(P, wsum_off); PUT(P, stage_off); PUT(P, stage_idx_off);
        PUT(P, total_bytes);
        j.put_layout("layout", P.layout);
        j.put_slot(P.slot, {{"pod_rows", P.slot_pods}, {"group_rows", P.slot_groups}});
    }
    j.emit();
    return 0;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (const int rc = plan_line(line)) return rc;
    }
    return 0;
}
