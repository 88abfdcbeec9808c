// sg_traffic_trend.h — K23: traffic baselines, an exponentially weighted baseline of the request RATE and the LOAD (busy time) per
// edge row, node row side, group edge and workload row side (include/servicegraph.h, "traffic baselines").  Included after
// sg_group_nodes.h: it reuses K8's walk (sg_trend.h), the sample sources of the four mean baselines (K8Edges, K10Nodes, K15Groups,
// K16Nodes), k8_scan and K7's passes unchanged.
//
// A traffic baseline is the mean baseline of its space with both samples swapped.  Keys, sample order, counts and the row layout
// are the base source's, so the window's samples are the same sorted list and the update is the same merge.  The samples read
// what the base's sample already holds — no further load, no division:
//
//   x_rate = 1000.0 * min(count, 2^42)      (the lat_* half; base_mean_us = (float)(mean / 1000) reads as requests per window)
//   x_load = (double) min(sum_ns, 2^52)     (the err_* half; requests x latency, the side's busy time)
//
// Both are exact integers in fp64: 1000 * 2^42 < 2^52.  A side with count 0 neither creates, refreshes nor scores an entry: the
// walk's own rule.
//
//   k23_ecount / k23_ewrite     K8's count and write pass over the window's rows    (K8's keys)
//   k23_ncount / k23_nwrite     ... over the node rows                              (K10's keys)
//   k23_gcount / k23_gwrite     ... over the group edges                            (K15's keys)
//   k23_wcount / k23_wwrite     ... over the workload rows                          (K16's keys)
//   k23_keys                    the key pass of the three selections by a traffic row, either sign
//
// k8_scan runs between each pair as it is; there is no vanished form.  The sources say flat_counts (sg_trend.h K8FlatCounts): the
// walk's counters stay in registers, no scratch.  K7's passes and k_gather_sel follow k23_keys unchanged.
#pragma once

// a sample source over Base (K8Edges, K10Nodes, K15Groups, K16Nodes): Args, Sample, count, sample, put and the keys are Base's.
// Base's sample has sum (u64) and count (u32 in K8Row, u64 in K10Sample)
template <class Base>
struct K23Traffic : Base {
    static constexpr bool flat_counts = true;
    static __device__ __forceinline__ double x_lat(const typename Base::Sample& r) {
        u64 c = r.count;
        if (c > (1ull << 42)) c = 1ull << 42;
        return 1000.0 * (double)c;
    }
    static __device__ __forceinline__ double x_err(const typename Base::Sample& r) {
        u64 s = r.sum;
        if (s > (1ull << 52)) s = 1ull << 52;
        return (double)s;
    }
};
typedef K23Traffic<K8Edges> K23Edges;
typedef K23Traffic<K10Nodes> K23Nodes;
typedef K23Traffic<K15Groups> K23Groups;
typedef K23Traffic<K16Nodes> K23Workloads;

__global__ __launch_bounds__(K8_THREADS) void k23_ecount(TrendArgs a) { k8_count_t<K23Edges, false>(a, a, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_ewrite(TrendArgs a) { k8_write_t<K23Edges, false>(a, a, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_ncount(NodeTrendArgs na) { k8_count_t<K23Nodes, false>(na.t, na, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_nwrite(NodeTrendArgs na) { k8_write_t<K23Nodes, false>(na.t, na, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_gcount(GroupTrendArgs ga) { k8_count_t<K23Groups, false>(ga.t, ga, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_gwrite(GroupTrendArgs ga) { k8_write_t<K23Groups, false>(ga.t, ga, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_wcount(NodeTrendArgs na) { k8_count_t<K23Workloads, false>(na.t, na, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k23_wwrite(NodeTrendArgs na) { k8_write_t<K23Workloads, false>(na.t, na, VanArgs{}); }

// ---- selection by a traffic row -----------------------------------------------------------------------------------------------
// k7_keys over traffic rows alone (k10_keys' shape): the key of word `word` of a row of `wpr` u32 words (4: sg_edge_trend, 8:
// sg_node_trend), its sign flipped when neg — a drop ranks by its size; -x of a NaN is a NaN, never a candidate, and k7_key maps
// both zeros to one key.  The entity rows are not read.  Workgroup 0 resets K7's state and copies the row count to
// ctr[C_N_EDGES], where K7's later passes read it (a.ctr = ctr).  i < E <= a.max_edges, the rows a slot's traffic rows hold.
__global__ __launch_bounds__(K7_THREADS) void k23_keys(SelArgs a, const u64* count, const u32* tw, u32 wpr, u32 word, u32 neg, u64* ctr) {
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
    const u32 flip = neg ? 0x80000000u : 0u;
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        const u32 key = k7_key(__uint_as_float(tw[i * wpr + word] ^ flip), a.min_score);
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}
