// sg_group_nodes.h — K16: the window's group edges rolled up per workload on the device, the per-workload baselines and the
// selection over workload rows (include/servicegraph.h, "workload rows").  Included after sg_group_trend.h: it reuses K9's fold
// helpers (K9Side, k9_zero .. k9_fetch, k9_block_excl_max), k9_scan, K8's walk and scan, k15_wk, k10_keys and K7's passes as they
// are, and adds kernels of its own beside them.
//
// A node is keyed by K14's group key: g for a group, max_groups + K9's node id otherwise — below GK = max_groups + ncap.  The group
// edges come out ascending by (gk(from), gk(to)), so a node's out edges are one run.  A group edge is already a fold of rows: it
// adds its sums, its maxima and its worst-row key (score key of score_max << 32 | ~worst_row) to a side, and 1 to the side's edges.
// Every field is an integer sum, an integer max or the max of a key: nothing depends on the order of the folds.  Five launches,
// K9's shape:
//
//   k16_out      k9_out's fold over the group edges: chunks of K9_CHUNK, K9_ROWS per thread; a run inside a span is stored by its
//                thread, a run cut by spans is folded in LDS, the (at most two) runs cut by the chunk's ends go to the table with
//                device-scope integer atomics.  Beside it dst[j] = gk(to_ref)
//   k16_in_part  k9_in_part's (range of K9_IN_NR keys x slice) pattern; ranges no node of the window can be in are skipped: K9's
//                used id ranges shifted by max_groups, and the group ranges below hi_group (one past the largest group id assigned)
//   k16_count    per key: the slices' partials summed into the in table; keys with group edges counted per workgroup
//   k9_scan      (sg_nodes.h, unchanged, on the embedded NodesArgs) the scan of the counts, the node count of the window
//   k16_write    the workload rows in key order; the out table entries it read are zeroed for the next window
//
// The baseline is K10's with the workload key of K15 (K16Nodes: k.f = k15_wk(ref)): ascending gk is ascending wk, so the window's
// 2 N samples are strictly ascending.  The selection is k10_keys, K7's passes and k_gather_sel<sg_node_out>: no kernel of its own.
#pragma once

struct GroupNodesArgs {
    NodesArgs nd;                 // ctr and the id spaces (k9_node, k9_ref, k9_used); slices, node_per, dst, tout, tin, part over GK
                                  // keys; blk and count for k9_scan; out: this window's workload rows
    const sg_group_edge* groups;  // the window's group edges (K14)
    const u64* gcount;            // their count
    u32 max_groups, gk;           // GK = max_groups + ncap
    u32 hi_group;                 // one past the largest group id assigned since sg_set_groups
    u32 nc;                       // the workload rows a window can have
};

__device__ __forceinline__ u64 k16_edges_of(const GroupNodesArgs& a) { const u64 E = *a.gcount; return E < a.nd.max_edges ? E : a.nd.max_edges; }
// the group key of a group ref (SG_NONE: a ref beyond the id spaces, no window has one)
__device__ __forceinline__ u32 k16_gk(const GroupNodesArgs& a, u32 ref) {
    if (SG_REF_TYPE(ref) == SG_REF_GROUP) { const u32 g = SG_REF_VALUE(ref); return g < a.max_groups ? g : SG_NONE; }
    const u32 k = k9_node(a.nd, ref);
    return k == SG_NONE ? SG_NONE : a.max_groups + k;
}
__device__ __forceinline__ u32 k16_from(const GroupNodesArgs& a, u64 j) { return k16_gk(a, (u32)reinterpret_cast<const u64*>(a.groups + j)[6]); }
// what a group edge adds to a side, and its refs: the 80-byte row as five 16-byte loads
struct K16Row { K9Side s; u32 from, to; };
__device__ __forceinline__ K16Row k16_load(const GroupNodesArgs& a, u64 j) {
    const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.groups + j);
    const ulonglong2 w0 = r[0], w1 = r[1], w2 = r[2], w3 = r[3], w4 = r[4];
    K16Row o;
    o.s.cnt = w0.x; o.s.err = w0.y; o.s.sum = w1.x; o.s.ssq = w1.y; o.s.max = w2.x; o.s.q32 = w2.y;
    o.from = (u32)w3.x; o.to = (u32)(w3.x >> 32);
    o.s.alive = (u32)(w4.x >> 32);
    o.s.worst = ((u64)k9_score_key(__uint_as_float((u32)(w4.y >> 32))) << 32) | (u64)(~(u32)w4.y);
    o.s.edges = 1u;
    return o;
}
// the keys this window can hold: the groups below hi_group, K9's used ids shifted by max_groups
__device__ __forceinline__ bool k16_in_used(const GroupNodesArgs& a, const K9Used& u, u32 v) {
    return v < a.max_groups ? v < a.hi_group : k9_in_used(u, v - a.max_groups);
}
__device__ __forceinline__ bool k16_range_used(const GroupNodesArgs& a, const K9Used& u, u32 n0, u32 n1) {   // [n0, n1) meets one of them
    if (n0 < a.hi_group) return true;
    if (n1 <= a.max_groups) return false;
    return k9_range_used(u, (n0 > a.max_groups ? n0 : a.max_groups) - a.max_groups, n1 - a.max_groups);
}

__global__ __launch_bounds__(K9_THREADS) void k16_out(GroupNodesArgs a) {
    // slot b: the run whose first crossed span boundary is b (0 = the chunk's start: a run that began in an earlier chunk)
    __shared__ K9Side slot[K9_THREADS + 1];
    __shared__ u32 snode[K9_THREADS + 1];
    __shared__ u32 wmax[K9_THREADS / 64];
    __shared__ u32 tail_slot, tail_out;
    const u64 E = k16_edges_of(a);
    const u64 c0 = (u64)blockIdx.x * K9_CHUNK;
    if (c0 >= E) return;                                             // (uniform)
    const u64 c1 = c0 + K9_CHUNK < E ? c0 + K9_CHUNK : E;
    const u32 t = threadIdx.x;
    for (u32 s = t; s <= K9_THREADS; s += K9_THREADS) { k9_zero(slot[s]); snode[s] = SG_NONE; }
    const u64 j0 = c0 + (u64)t * K9_ROWS;
    const u32 n = j0 < c1 ? (u32)((c1 - j0) < K9_ROWS ? (c1 - j0) : K9_ROWS) : 0u;
    const u64 j1 = j0 + n;
    K9Side r[K9_ROWS];
    u32 f[K9_ROWS];
#pragma unroll
    for (int q = 0; q < K9_ROWS; q++) {
        if ((u32)q < n) {
            const K16Row x = k16_load(a, j0 + q);
            r[q] = x.s;
            f[q] = k16_gk(a, x.from);
            a.nd.dst[j0 + q] = k16_gk(a, x.to);
        } else {
            f[q] = SG_NONE;
        }
    }
    const u32 fprev = (n && j0 > 0) ? k16_from(a, j0 - 1) : SG_NONE;
    const u32 fnext = (n && j1 < E) ? k16_from(a, j1) : SG_NONE;
    const bool first_head = n && (j0 == 0 || fprev != f[0]);         // a run begins at j0
    bool any_head = first_head;
#pragma unroll
    for (int q = 1; q < K9_ROWS; q++) any_head |= (u32)q < n && f[q] != f[q - 1];
    const u32 before = k9_block_excl_max<K9_THREADS>(any_head ? t + 1 : 0u, wmax);   // (its __syncthreads also orders the slot init)
    const u32 slot_first = first_head ? t + 1 : before;             // the slot of the run that holds j0, if it is cut
    if (n) {
        K9Side acc; k9_zero(acc);
        bool here = first_head;                                      // the current run began inside this span
        u32 cur = f[0];
        auto fold = [&](bool cut, u32 s) {
            if (cur == SG_NONE) return;
            if (!cut) { k9_store(a.nd.tout + cur, acc); return; }    // the whole run is in this span: its only writer
            k9_atomic_merge(&slot[s], acc);
            snode[s] = cur;
        };
#pragma unroll
        for (int q = 0; q < K9_ROWS; q++) {
            if ((u32)q >= n) break;
            if (q > 0 && f[q] != f[q - 1]) {
                fold(!here, slot_first);
                k9_zero(acc); cur = f[q]; here = true;
            }
            k9_merge(acc, r[q]);
        }
        const bool flows = j1 < E && fnext == cur;                   // the last run goes on past this span
        fold(flows || !here, here ? t + 1 : slot_first);
        if (j1 == c1) { tail_slot = here ? t + 1 : slot_first; tail_out = flows ? 1u : 0u; }
    }
    __syncthreads();
    for (u32 s = t; s <= K9_THREADS; s += K9_THREADS) {
        const u32 v = snode[s];
        if (v == SG_NONE) continue;
        if (s == 0 || (s == tail_slot && tail_out)) k9_atomic_merge(a.nd.tout + v, slot[s]);   // shared with a neighbouring chunk
        else k9_store(a.nd.tout + v, slot[s]);
    }
}

__global__ __launch_bounds__(K9_IN_THREADS) void k16_in_part(GroupNodesArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    K9Side* acc = reinterpret_cast<K9Side*>(smem);
    const u32 S = a.nd.slices, g = blockIdx.x, t = threadIdx.x;
    const u32 rg = g / S, sl = g % S, n0 = rg * K9_IN_NR;
    if (n0 >= a.gk) return;
    const u32 nr = a.gk - n0 < K9_IN_NR ? a.gk - n0 : K9_IN_NR;
    if (!k16_range_used(a, k9_used(a.nd), n0, n0 + nr)) return;     // (k16_count reads no partial of such a range)
    for (u32 i = t; i < nr; i += K9_IN_THREADS) k9_zero(acc[i]);
    __syncthreads();
    const u64 E = k16_edges_of(a);
    const u64 per = (E + S - 1) / S, p0 = (u64)sl * per < E ? (u64)sl * per : E, p1 = p0 + per < E ? p0 + per : E;
    // K9_IN_Q group edges per thread and trip; the destinations of the next trip are fetched before this trip's group edges
    u32 nxt[K9_IN_Q];
#pragma unroll
    for (int q = 0; q < K9_IN_Q; q++) { const u64 p = p0 + t + (u64)q * K9_IN_THREADS; nxt[q] = p < p1 ? a.nd.dst[p] - n0 : 0xFFFFFFFFu; }
    for (u64 pb = p0 + t; pb < p1; pb += (u64)K9_IN_THREADS * K9_IN_Q) {
        u32 to[K9_IN_Q];
        K9Side x[K9_IN_Q];
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) { to[q] = nxt[q]; if (to[q] < nr) x[q] = k16_load(a, pb + (u64)q * K9_IN_THREADS).s; }
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) { const u64 p = pb + (u64)(K9_IN_Q + q) * K9_IN_THREADS; nxt[q] = p < p1 ? a.nd.dst[p] - n0 : 0xFFFFFFFFu; }
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) if (to[q] < nr) k9_atomic_merge(acc + to[q], x[q]);
    }
    __syncthreads();
    K9Side* out = a.nd.part + ((size_t)rg * S + sl) * K9_IN_NR;
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(acc);
    ulonglong2* dp = reinterpret_cast<ulonglong2*>(out);
    for (u32 i = t; i < nr * 4; i += K9_IN_THREADS) dp[i] = src[i];
}

// the workgroup's keys [v0, v1) in rounds of K9_THREADS
__device__ __forceinline__ void k16_key_span(const GroupNodesArgs& a, u32& v0, u32& v1) {
    v0 = blockIdx.x * a.nd.node_per; v1 = v0 + a.nd.node_per;
    if (v0 > a.gk) v0 = a.gk;
    if (v1 > a.gk) v1 = a.gk;
}

__global__ __launch_bounds__(K9_THREADS) void k16_count(GroupNodesArgs a) {
    __shared__ u32 ws[K9_THREADS / 64];
    const u32 t = threadIdx.x, S = a.nd.slices;
    const K9Used u = k9_used(a.nd);
    u32 v0, v1; k16_key_span(a, v0, v1);
    u32 c = 0;
    for (u32 v = v0 + t; v < v1; v += K9_THREADS) {
        K9Side in; k9_zero(in);
        if (k16_in_used(a, u, v)) {
            const u32 rg = v / K9_IN_NR, i = v - rg * K9_IN_NR;
            const K9Side* p = a.nd.part + (size_t)rg * S * K9_IN_NR + i;
            for (u32 sl = 0; sl < S; sl++) k9_merge(in, k9_fetch(p + (size_t)sl * K9_IN_NR));
        }
        k9_store(a.nd.tin + v, in);
        const u32 oe = reinterpret_cast<const u32*>(a.nd.tout + v)[14];   // (out edges: word 14 of the entry)
        c += (oe + in.edges) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if ((t & 63) == 0) ws[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        u32 k = 0;
        for (int w = 0; w < K9_THREADS / 64; w++) k += ws[w];
        a.nd.blk[blockIdx.x] = k;
    }
}

__global__ __launch_bounds__(K9_THREADS) void k16_write(GroupNodesArgs a) {
    __shared__ u32 wsum[K9_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    u32 v0, v1; k16_key_span(a, v0, v1);
    u32 base = a.nd.blk[K9_MAX_WGS + blockIdx.x];
    for (u32 vb = v0; vb < v1; vb += K9_THREADS) {                  // (uniform: every thread takes every round)
        const u32 v = vb + t;
        K9Side O, I;
        bool has = false;
        if (v < v1) { O = k9_fetch(a.nd.tout + v); I = k9_fetch(a.nd.tin + v); has = (O.edges + I.edges) != 0; }
        u32 tot;
        const u32 x = block_excl_scan<K9_THREADS>(has ? 1u : 0u, wsum, &tot);
        if (has) {
            sg_node_out o;
            o.out_count = O.cnt; o.in_count = I.cnt; o.out_err = O.err; o.in_err = I.err;
            o.out_sum_ns = O.sum; o.in_sum_ns = I.sum; o.out_sumsq_us = O.ssq; o.in_sumsq_us = I.ssq;
            o.out_max_ns = O.max; o.in_max_ns = I.max; o.out_score_q32 = O.q32; o.in_score_q32 = I.q32;
            o.ref = v < a.max_groups ? SG_MAKE_REF(SG_REF_GROUP, v) : k9_ref(a.nd, v - a.max_groups);
            o.out_edges = O.edges; o.in_edges = I.edges; o.out_alive = O.alive; o.in_alive = I.alive;
            o.out_worst_row = O.edges ? ~(u32)O.worst : 0xFFFFFFFFu; o.in_worst_row = I.edges ? ~(u32)I.worst : 0xFFFFFFFFu;
            o.out_score_max = O.edges ? k9_key_score((u32)(O.worst >> 32)) : 0.0f;
            o.in_score_max = I.edges ? k9_key_score((u32)(I.worst >> 32)) : 0.0f;
            o.score = o.out_score_max > o.in_score_max ? o.out_score_max : o.in_score_max;
            if (base + x < a.nc) a.nd.out[base + x] = o;             // (a window has at most min(GK, 2 E) nodes: the test keeps a stray count inside the buffer)
            if (O.edges) { K9Side z; k9_zero(z); k9_store(a.nd.tout + v, z); }   // the out side adds into a zero table
        }
        base += tot;
    }
}

// ---- the per-workload baselines -------------------------------------------------------------------------------------------------
// K10's sample source with K15's workload key: sample j = 2 * row + side, key (wk(ref), side)
struct K16Nodes : K10Nodes {
    static __device__ __forceinline__ K10Sample sample(const NodeTrendArgs& a, u64 j, u32 nob) {
        K10Sample o = k10_sample(a, j, nob);
        o.k.f = k15_wk(reinterpret_cast<const u32*>(a.nodes + (j >> 1))[24], a.t.ob_sorted, nob);   // ref: byte 96
        return o;
    }
};

__global__ __launch_bounds__(K8_THREADS) void k16_tcount(NodeTrendArgs na) { k8_count_t<K16Nodes, false>(na.t, na, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k16_twrite(NodeTrendArgs na) { k8_write_t<K16Nodes, false>(na.t, na, VanArgs{}); }
