// sg_group_trend.h — K15: per-workload-edge latency / error baselines kept across windows on the device, their vanished list and
// the selection over a window's group edges (include/servicegraph.h, "groups").  Included after sg_group.h: it reuses the helpers
// of sg_sel.h, sg_trend.h and sg_node_trend.h and their kernels unchanged (k8_scan, k8_scan_v, K7's pick / count / scan / scatter /
// sort), and adds kernels of its own beside them.
//
// A window's group edges (K14) come out ascending by (gk(from), gk(to)).  The workload key wk of a group ref — g for a group, else
// (1 + type) << 32 | x with x the ref's value, the IPv4 address for an OBIP ref (k8_ref_key, one type up) — ascends as gk does: the
// groups by id, then the ungrouped KNOWN nodes by id, then LABEL, then OBIP (whose indices follow the ascending outbound-IP list).
// Distinct group edges have distinct (gk, gk), so the window's group edges are strictly ascending in (wk(from_ref), wk(to_ref)): a
// sorted sample list, and the update is K8's merge of the old entries with it — K8's own walk (sg_trend.h) over the sample source
// K15Groups below:
//
//   k15_count  K8's count pass: merge-path split, one span per thread; the walk writes every group edge's sg_edge_trend (it needs
//              only the prior entry) and counts the kept old entries and the new ones
//   k8_scan    (1 workgroup, K8's kernel on the TrendArgs part) scans, the capacity cut, the new B and the statistics
//   k15_write  K8's write pass: merged, updated, unexpired entries into the other buffer, in key order
//
// k15_count_v / k8_scan_v / k15_write_v are the same with the vanished list (sg_set_group_vanished).  A group edge with count 0 (it
// folds alive-only rows only) is a sample that neither creates nor refreshes an entry, as K8's alive-only rows.  The counts are u64,
// so the samples are K10's: min(sum / count, 2^52) and the long division of err * 2^20 / count.
//
// Selection is K7 with a key pass of its own (k15_keys: the group edge's score_max or a value of its sg_edge_trend) over a count
// the key pass copies to word C_N_EDGES of a small counter block; K7's passes then select indices only (their row copies are off),
// and k_gather_sel<sg_group_edge> (sg_kernels.h) copies the selected group edges.  No K7, K8, K10 or K14 kernel changes.
#pragma once

struct GroupTrendArgs {
    TrendArgs t;                  // K8's part: ctr (C_N_OBIP), ob_sorted, max_obip, cap, buf, th, blk, ctl, w, warmup, ttl, alpha, floors
    const sg_group_edge* groups;  // the window's group edges (K14, ascending by group key pair)
    const u64* count;             // their count
    u64 max_edges;                // the group edges a window can have
    sg_edge_trend* out;           // [max_edges] this window's group trend rows
};

// the workload key of a group ref
__device__ __forceinline__ u64 k15_wk(u32 ref, const u32* ob, u32 nob) {
    if (SG_REF_TYPE(ref) == SG_REF_GROUP) return (u64)SG_REF_VALUE(ref);
    return k8_ref_key(ref, ob, nob) + (1ull << 32);
}
// group edge j as a sample: count, err_count, sum_ns (words 0 - 2 of the 80-byte row) and from_ref | to_ref << 32 (word 6)
__device__ __forceinline__ K10Sample k15_sample(const GroupTrendArgs& a, u64 j, u32 nob) {
    const u64* r = reinterpret_cast<const u64*>(a.groups + j);
    const u64 refs = r[6];
    K10Sample o;
    o.count = r[0]; o.err = r[1]; o.sum = r[2];
    o.k.f = k15_wk((u32)refs, a.t.ob_sorted, nob); o.k.t = k15_wk((u32)(refs >> 32), a.t.ob_sorted, nob);
    return o;
}

// K15's sample source for K8's walk: the window's min(count, max_edges) group edges, one sg_edge_trend each
struct K15Groups {
    typedef GroupTrendArgs Args;
    typedef K10Sample Sample;
    static __device__ __forceinline__ u64 count(const GroupTrendArgs& a, u64) { const u64 N = *a.count; return N < a.max_edges ? N : a.max_edges; }
    static __device__ __forceinline__ K10Sample sample(const GroupTrendArgs& a, u64 j, u32 nob) { return k15_sample(a, j, nob); }
    static __device__ __forceinline__ double x_lat(const K10Sample& r) { return k10_x_lat(r); }
    static __device__ __forceinline__ double x_err(const K10Sample& r) { return k10_x_err(r); }
    static __device__ __forceinline__ void put(const GroupTrendArgs& a, u64 j, float ld, float ed, float base, u32 seen) {
        sg_edge_trend t; t.lat_dev = ld; t.err_dev = ed; t.base_mean_us = base; t.windows_seen = seen;
        a.out[j] = t;
    }
};

__global__ __launch_bounds__(K8_THREADS) void k15_count(GroupTrendArgs ga) { k8_count_t<K15Groups, false>(ga.t, ga, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k15_write(GroupTrendArgs ga) { k8_write_t<K15Groups, false>(ga.t, ga, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k15_count_v(GroupTrendArgs ga, VanArgs v) { k8_count_t<K15Groups, true>(ga.t, ga, v); }
__global__ __launch_bounds__(K8_THREADS) void k15_write_v(GroupTrendArgs ga, VanArgs v) { k8_write_t<K15Groups, true>(ga.t, ga, v); }

// ---- selection over group edges -----------------------------------------------------------------------------------------------
// k7_keys over group edges: the key of the group edge's score_max (byte 76 of an 80-byte row) or of a value of its sg_edge_trend
// (SG_SEL_LAT_DEV: word 0 of 4, SG_SEL_ERR_DEV: word 1), or for SG_SEL_NEW one key for every group edge with windows_seen == 0 and
// count > 0.  Workgroup 0 copies the group-edge count to ctr[C_N_EDGES], where K7's later passes read it (a.ctr = ctr).
__global__ __launch_bounds__(K7_THREADS) void k15_keys(SelArgs a, const sg_group_edge* groups, const u64* count, const sg_edge_trend* tr,
                                                       u32 by, u64* ctr) {
    __shared__ u32 h[256];
    const u32 t = threadIdx.x;
    h[t] = 0;
    const u64 N = *count;
    if (blockIdx.x == 0 && t == 0) {
        a.state[K7S_PREFIX] = 0; a.state[K7S_REM] = a.k; a.state[K7S_DONE] = a.k == 0 ? 1u : 0u; a.state[K7S_SEL] = 0;
        ctr[C_N_EDGES] = N;
    }
    __syncthreads();
    const u64 E = N < a.max_edges ? N : a.max_edges;
    u64 lo, hi; k7_span(E, lo, hi);
    const u32* tw = reinterpret_cast<const u32*>(tr);                      // 4 words per trend row
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        u32 key;
        if (by == SG_SEL_SCORE) key = k7_key(groups[i].score_max, a.min_score);
        else if (by == SG_SEL_NEW) key = tw[i * 4 + 3] == 0u && groups[i].count > 0ull ? 0x80000000u : 0u;
        else key = k7_key(__uint_as_float(tw[i * 4 + (by == SG_SEL_ERR_DEV ? 1u : 0u)]), a.min_score);
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}
