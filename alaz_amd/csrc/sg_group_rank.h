// sg_group_rank.h — K17: each window's likely root-cause workloads ranked on the device (include/servicegraph.h, "workload ranking").
// Included after sg_group_nodes.h: it reuses K16's group key (k16_gk), K11's seed rule (k11_seed_of), K11's edge pass (k_rank_edge_t,
// over K17Space below), k11_keys, K7's passes and the gathers unchanged, and adds kernels of its own.
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
//   k17_edge    k11_edge's body over row indices: workgroup (range, slice) holds K17_NR u64 accumulators in LDS (8192 rows = 64 KiB:
//               two workgroups a CU) and scans its slice of the group edges; BY_SRC: acc[src] += w (the out-weight W, once a window);
//               else acc[dst] += t[src] * w (once an iteration) with LDS integer atomics.  A range at or beyond the window's row count
//               exits; the partial written is min(K17_NR, n - n0) words
//   k17_node    per workload row: k11_node's arithmetic, indexed by row.  With up to 256 slices the sum of a row's partials is the
//               pass's work, so a workgroup takes K17_NODE_ROWS rows at a time and K17_NODE_SPLIT threads share a row's slices
//               (consecutive threads read consecutive rows: 256 B a slice); the sums meet in LDS and the first thread of a row
//               does the rest.  Integer adds: the result does not depend on the split
#pragma once

#define K17_THREADS 256           // k17_pos, k17_prep, k17_node
#define K17_NR 8192               // rows per range: 8192 x 8 B = 64 KiB of LDS (k17_edge: K11_EDGE_THREADS threads, K11_Q group edges a trip)
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

// (k17_pos + k17_prep stay K17's own against k11_prep: the rows' positions must be complete before a group edge can look them up)
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
        sum += k11_seed_of(a.seed, a.seed_min, nrow->score);
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

// K17's space for K11's edge pass (sg_rank.h): ranges of K17_NR row indices, and only those below the window's row count run
struct K17Space {
    typedef GroupRankArgs Args;
    static constexpr u32 NR = K17_NR;
    static constexpr bool SKIP_T_OF_ZERO_W = true;
    static __device__ __forceinline__ u64 edges(const GroupRankArgs& a) { return k16_edges_of(a.g); }
    static __device__ __forceinline__ bool range(const GroupRankArgs& a, u32 rg, u32& n0, u32& nr) {
        const u64 N = k17_rows_of(a), first = (u64)rg * K17_NR;
        if (first >= N) return false;
        n0 = (u32)first; nr = N - first < K17_NR ? (u32)(N - first) : K17_NR;
        return true;
    }
};
template <bool BY_SRC>
__global__ __launch_bounds__(K11_EDGE_THREADS) void k17_edge(GroupRankArgs a) { k_rank_edge_t<K17Space, BY_SRC>(a); }

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

// (k17_node stays K17's own: it works by row and eight threads share a row's slices; k11_node goes through k9_node, a thread a row)
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
            const u64 av = A ? k11_seed_of(a.seed, a.seed_min, a.nodes[v].score) : 1ull;   // A == 0: the uniform seed
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
