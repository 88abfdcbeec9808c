// The CPU driver of plan_slo (alaz_amd/csrc/sg_plan.hpp) for tests/test_slo_host.py: one JSON object per input line.
//   slo_plan_test plan       "spaces on mk ml max_groups ncap nc slots struct_size latency_bin latency_target_ppm error_target_ppm
//                             short_windows long_windows min_burn_q10 reserved min_requests": plan_slo's verdict, the budgets and "sp"
//                             over [nodes, workloads] (null: the space is off) with each block's layout
//   slo_plan_test objective  "word": whether sg_slo_assign admits the word, its bin and its two budgets in ppm (0: a code that is none)
#include <iostream>

#include "plan_json.hpp"

using namespace sgplan;
typedef unsigned long long ull;

static int plan_line(const std::string& line) {
    std::istringstream is(line);
    ull v[17] = {};
    for (ull& x : v) if (!(is >> x)) { std::fprintf(stderr, "slo_plan_test: 17 numbers a line: %s\n", line.c_str()); return 2; }
    sg_slo_params p{};
    p.struct_size = (u32)v[8]; p.latency_bin = (u32)v[9]; p.latency_target_ppm = (u32)v[10]; p.error_target_ppm = (u32)v[11];
    p.short_windows = (u32)v[12]; p.long_windows = (u32)v[13]; p.min_burn_q10 = (u32)v[14]; p.reserved = (u32)v[15]; p.min_requests = v[16];
    SloPlan P;
    const int rc = plan_slo(p, (u32)v[0], (u32)v[1], v[2], v[3], v[4], (u32)v[5], (u32)v[6], (u32)v[7], &P);
    Json j;
    j.kv("rc", rc).kv("slots", v[7]).kv("params_size", sizeof(sg_slo_params)).kv("stats_size", sizeof(sg_slo_stats));
    j.kv("row_words", SG_SLO_WORDS).kv("entry_words", SG_SLO_ENTRY_WORDS).kv("max_windows", SG_SLO_MAX_WINDOWS).kv("stage_rows", kSloStageRows);
    if (rc == SG_OK) {
        PUT(P, spaces); PUT(P, lat_budget); PUT(P, err_budget); PUT(P, total_bytes);
        j.arr("sp");
        for (u32 k = 0; k < kSloSpaces; k++) {
            const SloSpace& s = P.sp[k];
            if (!s.on) { j.null(); continue; }
            j.obj();
            PUT(s, keys); PUT(s, cap); PUT(s, key_wgs); PUT(s, row_wgs); PUT(s, ring_bytes); PUT(s, sums_bytes); PUT(s, obj_bytes); PUT(s, rows_bytes);
            PUT(s, ring_off); PUT(s, sums_off); PUT(s, obj_off); PUT(s, ctl_off); PUT(s, stage_off); PUT(s, stage_idx_off); PUT(s, total_bytes);
            j.put_layout("layout", s.layout);
            j.put_slot(s.slot, {{"rows", s.slot_rows}});
            j.end();
        }
        j.end();
    }
    j.emit();
    return 0;
}

static int objective_line(const std::string& line) {
    const u32 w = (u32)std::strtoull(line.c_str(), nullptr, 0);
    Json j;
    j.kv("word", w).kv("ok", slo_objective_ok(w)).kv("bin", w >> 28).kv("lat_budget", slo_budget(w >> 12 & 0xFFFu)).kv("err_budget", slo_budget(w & 0xFFFu));
    j.emit();
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode != "plan" && mode != "objective") { std::fprintf(stderr, "usage: slo_plan_test plan|objective < lines\n"); return 2; }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (const int rc = mode == "plan" ? plan_line(line) : objective_line(line)) return rc;
    }
    return 0;
}
