// sg_group_rank.h — K17: each window's likely root-cause workloads ranked on the device (include/servicegraph.h, "workload ranking").
// Included after sg_group_nodes.h: it reuses K16's group key (k16_gk), K11's seed rule (k11_seed_of's q16), k11_keys, K7's passes and
// the gathers unchanged, and adds kernels of its own.
//
// K11's walk with "row" read as "group edge" and "node row" read as "workload row", in u64 integer arithmetic only.  K11 works in
// node-key space; K16's rows are dense and ascending by group key, so this stage works in ROW-INDEX space: every per-node array is
// [NC] by row position, read and written coalesced, and the (range x slice) accumulation only runs the ranges below the window's row
// count.  pos, src, dst and w are the stage's own (K16's scratch is shared by the slots: the next slot's K16 may run while this
// slot's iterations still read).  Only the window's keys of pos are written and only those are read, so nothing is zeroed between
// windows.  2 * iters + 4 plain launches on the window's stream:
//
//   k17_pos     per workload row v: pos[gk(ref_v)] = v; the seed a_v, summed per workgroup
//   k17_prep    per group edge j: src[j] = pos[gk(from)], dst[j] = pos[gk(to)] and the weight w[j] = edges + min(score_q32 >> 16,
//               65536 * edges) as a u64 (16 bytes a group edge for the iterations instead of the 80-byte rows)
//   k17_edge    k11_edge's pattern over row indices: workgroup (range, slice) holds K17_NR u64 accumulators in LDS (8192 rows = 64 KiB:
//               two workgroups a CU) and scans its slice of the group edges; BY_SRC: acc[src] += w (the out-weight W, once a window);
//               else acc[dst] += t[src] * w (once an iteration) with LDS integer atomics.  A range at or beyond the window's row count
//               exits; the partial written is min(K17_NR, n - n0) words
//   k17_node    per workload row: k11_node's arithmetic, indexed by row.  With up to 256 slices the sum of a row's partials is the
//               pass's work, so a workgroup takes K17_NODE_ROWS rows at a time and K17_NODE_SPLIT threads share a row's slices
//               (consecutive threads read consecutive rows: 256 B a slice); the sums meet in LDS and the first thread of a row
//               does the rest.  Integer adds: the result does not depend on the split
#pragma once

#define K17_THREADS 256           // k17_pos, k17_prep, k17_node
#define K17_EDGE_THREADS 1024     // k17_edge
#define K17_NR 8192               // rows per range: 8192 x 8 B = 64 KiB of LDS
#define K17_Q 4                   // group edges per thread and trip of k17_edge
#define K17_MAX_WGS 1024          // k17_pos's grid at most (k17_node sums one seed sum per workgroup)
#define K17_NODE_ROWS 32          // rows per workgroup and round of k17_node
#define K17_NODE_SPLIT (K17_THREADS / K17_NODE_ROWS)   // threads that share a row's slices

struct GroupRankArgs {
    GroupNodesArgs g;             // K16's part: the id spaces, max_edges, groups, gcount, max_groups, gk, nc (k16_gk, k16_edges_of)
    const sg_node_out* nodes;     // the window's workload rows
    const u64* count;             // their count
    u32 slices, pos_wgs;          // group-edge slices of k17_edge; workgroups of k17_pos
    u32 damping, seed;            // D in 1..255; SG_RANK_SEED_*
    float seed_min;
    u32* pos;                     // [GK] row position by group key (the window's keys only)
    u32* src; u32* dst; u64* w;   // [max_edges] per group edge: row positions and weight
    u64* W; u64* R; u64* base; u64* t;   // [NC] by row position
    u64* part;                    // [ranges][slices][K17_NR] per-slice partials
    u64* seed_sum;                // [K17_MAX_WGS] per workgroup of k17_pos
    sg_node_rank* out;            // [NC] this window's rank rows
};

__device__ __forceinline__ u64 k17_rows_of(const GroupRankArgs& a) { return sg_nodes_of(a.count, a.g.nc); }
__device__ __forceinline__ u64 k17_seed_of(const GroupRankArgs& a, float score) {
    if (a.seed == SG_RANK_SEED_UNIFORM) return 1ull;
    return score >= a.seed_min ? (u64)k11_q16(score) : 0ull;
}

__global__ __launch_bounds__(K17_THREADS) void k17_pos(GroupRankArgs a) {
    __shared__ u64 ssum;
    const u32 t = threadIdx.x;
    if (t == 0) ssum = 0;
    __syncthreads();
    const u64 N = k17_rows_of(a);
    u64 sum = 0;
    for (u64 v = (u64)blockIdx.x * K17_THREADS + t; v < N; v += (u64)gridDim.x * K17_THREADS) {
        const sg_node_out* nrow = a.nodes + v;
        const u32 k = k16_gk(a.g, nrow->ref);
        if (k != SG_NONE && k < a.g.gk) a.pos[k] = (u32)v;           // (cannot fail: K16 made the row from such a key)
        sum += k17_seed_of(a, nrow->score);
    }
    if (sum) atomicAdd(&ssum, sum);
    __syncthreads();
    if (t == 0) a.seed_sum[blockIdx.x] = ssum;
}

__global__ __launch_bounds__(K17_THREADS) void k17_prep(GroupRankArgs a) {
    const u64 G = k16_edges_of(a.g), N = k17_rows_of(a);
    for (u64 j = (u64)blockIdx.x * K17_THREADS + threadIdx.x; j < G; j += (u64)gridDim.x * K17_THREADS) {
        const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.g.groups + j);   // (k16_load's words: score_q32, from | to << 32, edges)
        const ulonglong2 w2 = r[2], w3 = r[3];
        const u64 edges = (u32)w3.y, q = w2.y >> 16, top = 65536ull * edges;
        u64 w = edges + (q < top ? q : top);
        const u32 fk = k16_gk(a.g, (u32)w3.x), tk = k16_gk(a.g, (u32)(w3.x >> 32));
        u32 s = 0, d = 0;
        if (fk == SG_NONE || tk == SG_NONE || fk >= a.g.gk || tk >= a.g.gk) w = 0;   // (a ref beyond the id spaces has no row: the group edge carries nothing)
        else { s = a.pos[fk]; d = a.pos[tk]; }
        if (s >= N || d >= N) { s = 0; d = 0; w = 0; }                // (a row count beyond the slot's capacity: the rows cut have no position)
        a.src[j] = s; a.dst[j] = d; a.w[j] = w;
    }
}

template <bool BY_SRC>
__global__ __launch_bounds__(K17_EDGE_THREADS) void k17_edge(GroupRankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* acc = reinterpret_cast<u64*>(smem);
    const u32 S = a.slices, g = blockIdx.x, t = threadIdx.x;
    const u32 rg = g / S, sl = g % S;
    const u64 N = k17_rows_of(a), n0 = (u64)rg * K17_NR;
    if (n0 >= N) return;                                             // (uniform: k17_node reads no partial of such a range)
    const u32 nr = N - n0 < K17_NR ? (u32)(N - n0) : K17_NR;
    for (u32 i = t; i < nr; i += K17_EDGE_THREADS) acc[i] = 0;
    __syncthreads();
    const u64 G = k16_edges_of(a.g);
    const u64 per = (G + S - 1) / S, p0 = (u64)sl * per < G ? (u64)sl * per : G, p1 = p0 + per < G ? p0 + per : G;
    const u32* key = BY_SRC ? a.src : a.dst;
    for (u64 pb = p0 + t; pb < p1; pb += (u64)K17_EDGE_THREADS * K17_Q) {
        u32 k[K17_Q];
#pragma unroll
        for (int q = 0; q < K17_Q; q++) { const u64 p = pb + (u64)q * K17_EDGE_THREADS; k[q] = p < p1 ? key[p] - (u32)n0 : 0xFFFFFFFFu; }
#pragma unroll
        for (int q = 0; q < K17_Q; q++) if (k[q] < nr) {
            const u64 p = pb + (u64)q * K17_EDGE_THREADS;
            const u64 w = a.w[p];
            const u64 x = BY_SRC ? w : (w ? a.t[a.src[p]] * w : 0ull);   // (group edges ascend by source: t[src] is a cached, mostly uniform load)
            if (x) atomicAdd(&acc[k[q]], x);
        }
    }
    __syncthreads();
    u64* out = a.part + ((size_t)rg * S + sl) * K17_NR;
    for (u32 i = t; i < nr; i += K17_EDGE_THREADS) out[i] = acc[i];
}

// the partials of row v in the slices first, first + K17_NODE_SPLIT, ... summed
__device__ __forceinline__ u64 k17_part_sum(const GroupRankArgs& a, u64 v, u32 first) {
    const u64 rg = v / K17_NR, i = v - rg * K17_NR;
    const u32 S = a.slices;
    const u64* p = a.part + (size_t)rg * S * K17_NR + i;
    u64 s = 0;
#pragma unroll 8
    for (u32 sl = first; sl < S; sl += K17_NODE_SPLIT) s += p[(size_t)sl * K17_NR];
    return s;
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(K17_THREADS) void k17_node(GroupRankArgs a) {
    __shared__ u64 sA;
    __shared__ u64 sp[K17_NODE_SPLIT][K17_NODE_ROWS];
    const u32 t = threadIdx.x, lr = t % K17_NODE_ROWS, g = t / K17_NODE_ROWS;
    const u64 N = k17_rows_of(a);
    u64 A = 0;
    if (FIRST) {
        if (t == 0) sA = 0;
        __syncthreads();
        u64 s = 0;
        for (u32 i = t; i < a.pos_wgs; i += K17_THREADS) s += a.seed_sum[i];
        if (s) atomicAdd(&sA, s);
        __syncthreads();
        A = sA;
    }
    const u64 D = a.damping, M = 1ull << K11_M_LOG2;
    for (u64 b0 = (u64)blockIdx.x * K17_NODE_ROWS; b0 < N; b0 += (u64)gridDim.x * K17_NODE_ROWS) {   // (uniform: every thread takes every round)
        const u64 v = b0 + lr;
        sp[g][lr] = v < N ? k17_part_sum(a, v, g) : 0ull;
        __syncthreads();
        u64 ps = 0;
        if (g == 0) {
#pragma unroll
            for (u32 k = 0; k < K17_NODE_SPLIT; k++) ps += sp[k][lr];
        }
        __syncthreads();                                             // (the next round writes sp again)
        if (g != 0 || v >= N) continue;
        u64 r, W = 0, R = 0;
        if (FIRST) {
            const u64 av = A ? k17_seed_of(a, a.nodes[v].score) : 1ull;   // A == 0: the uniform seed
            const u64 p = av * (M / (A ? A : N));
            W = ps;
            R = (p >> 8) * (256 - D);
            a.W[v] = W; a.R[v] = R;
            r = p;
        } else {
            r = a.base[v] + ps;
        }
        if (LAST) {
            sg_node_rank o;
            o.rank = r; o.ref = a.nodes[v].ref; o.share = (float)((double)r * 0x1p-56);
            a.out[v] = o;
        } else {
            if (!FIRST) { W = a.W[v]; R = a.R[v]; }
            const u64 m = (r >> 8) * D, tt = W ? m / W : 0ull;
            a.t[v] = tt;
            a.base[v] = R + (m - tt * W);
        }
    }
}
