// sg_quantile_trend.h — K21: tail baselines, an exponentially weighted baseline of ONE tracked quantile per node row side, group
// edge and workload row side (include/servicegraph.h, "tail baselines").  Included after sg_quantiles.h: it reuses K8's walk
// (sg_trend.h), the sample sources of the three mean baselines (K10Nodes, K15Groups, K16Nodes) and k8_scan unchanged.
//
// A tail baseline is the mean baseline of its space with one thing swapped: the latency sample.  Keys, sample order, counts, the
// error sample and the row layout are the base source's, so the window's samples are the same sorted list and the update is the
// same merge.  x_lat = 1000.0 * Q, Q the u32 microsecond value K20 wrote for the tracked per-mille of the entity and side in this
// window (the slot's quantile table of the space: SG_Q_MAX words an entity and side, the tracked one at word qi).  Q < 2^32, so
// x_lat < 2^52 is exact in fp64.
//
// Side order: K20's tables hold a node's sides as [0] = out, [1] = in; K10's samples are side 0 = in, 1 = out.  Sample j = 2 * row +
// s reads K20 side 1 - s: word ((j >> 1) * 2 + (1 - s)) * SG_Q_MAX + qi.  The group edges have one side: word j * SG_Q_MAX + qi.
//
//   k21_ncount / k21_nwrite     K8's count and write pass over the node rows        (K10's keys)
//   k21_gcount / k21_gwrite     ... over the group edges                            (K15's keys)
//   k21_wcount / k21_wwrite     ... over the workload rows                          (K16's keys)
//
// k8_scan runs between the two as it is.  The selections by a tail row launch k10_keys / k15_keys, K7's passes and k_gather_sel
// unchanged, with the tail rows as tr.  No new key kernel, no scratch, no atomic.  The quantile load is bounded by the base
// source's count(): j < 2 min(count, ncap) or j < min(count, max_edges), and the slot's table holds SG_Q_MAX words for every entity
// and side up to that capacity (sg_plan.hpp plan_quantiles: the same ncap / max_edges / nc).
#pragma once

// the base source's argument, the slot's K20 table of the space and the tracked quantile's index in it
template <class BaseArgs>
struct QTrendArgs {
    BaseArgs b;
    const u32* quant;             // [entities][sides][SG_Q_MAX]
    u32 qi, pad;
};
typedef QTrendArgs<NodeTrendArgs> NodeQTrendArgs;
typedef QTrendArgs<GroupTrendArgs> GroupQTrendArgs;

// the base's sample and the loaded Q
struct K21Sample : K10Sample { u32 q; };

// a sample source over Base (K10Nodes, K15Groups, K16Nodes) with SIDES sides an entity: count, the key, x_err and put are Base's
template <class Base, u32 SIDES>
struct K21Tail {
    typedef QTrendArgs<typename Base::Args> Args;
    typedef K21Sample Sample;
    static constexpr bool flat_counts = true;                         // (sg_trend.h K8FlatCounts: the walk's counters stay in registers)
    static __device__ __forceinline__ u64 count(const Args& a, u64 edges) { return Base::count(a.b, edges); }
    static __device__ __forceinline__ K21Sample sample(const Args& a, u64 j, u32 nob) {
        K21Sample o;
        static_cast<K10Sample&>(o) = Base::sample(a.b, j, nob);
        const u64 w = SIDES == 2 ? (j ^ 1ull) : j;                    // (2 * row + (1 - s): K20's out / in against K10's in / out)
        o.q = a.quant[w * SG_Q_MAX + a.qi];
        return o;
    }
    static __device__ __forceinline__ double x_lat(const K21Sample& r) { return 1000.0 * (double)r.q; }
    static __device__ __forceinline__ double x_err(const K21Sample& r) { return Base::x_err(r); }
    static __device__ __forceinline__ void put(const Args& a, u64 j, float ld, float ed, float base, u32 seen) { Base::put(a.b, j, ld, ed, base, seen); }
};
typedef K21Tail<K10Nodes, 2> K21Nodes;
typedef K21Tail<K15Groups, 1> K21Groups;
typedef K21Tail<K16Nodes, 2> K21Workloads;

__global__ __launch_bounds__(K8_THREADS) void k21_ncount(NodeQTrendArgs qa) { k8_count_t<K21Nodes, false>(qa.b.t, qa, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k21_nwrite(NodeQTrendArgs qa) { k8_write_t<K21Nodes, false>(qa.b.t, qa, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k21_gcount(GroupQTrendArgs qa) { k8_count_t<K21Groups, false>(qa.b.t, qa, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k21_gwrite(GroupQTrendArgs qa) { k8_write_t<K21Groups, false>(qa.b.t, qa, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k21_wcount(NodeQTrendArgs qa) { k8_count_t<K21Workloads, false>(qa.b.t, qa, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k21_wwrite(NodeQTrendArgs qa) { k8_write_t<K21Workloads, false>(qa.b.t, qa, VanArgs{}); }
