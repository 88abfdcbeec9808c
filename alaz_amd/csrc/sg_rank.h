// sg_rank.h — K11: each window's likely root-cause services ranked on the device (include/servicegraph.h, "culprit ranking").
// Included after sg_node_trend.h: it reuses K9's node key (k9_node) and K7's selection passes unchanged, and adds kernels of its own.
//
// A random walk with restart over the window's rows, caller to callee, stepping along a row with probability proportional to
// 1 + q16(score), in u64 integer arithmetic only: every sum is an integer add, so the result has one value whatever order the
// workgroups and lanes run in.  Work is in K9's node-key space (k9_node(ref) < ncap); only the keys of the window's node rows are
// ever read or written, so nothing is zeroed between windows.  2 * iters + 3 plain launches on the window's stream:
//
//   k11_prep    per row: the source's and the destination's node key and the weight w = 1 + q16(score) into three u32 arrays (12
//               bytes a row for the iterations instead of the 64-byte rows); per node row: the seed a, summed per workgroup
//   k11_edge    k9_in_part's pattern: workgroup (range, slice) holds K11_NR u64 accumulators in LDS (16 384 nodes = 128 KiB) and
//               scans its slice of the rows; BY_SRC: acc[src] += w (the out-weight W, once a window); else acc[dst] += t[src] * w
//               (the mass handed along the rows, once an iteration) with LDS integer atomics; it writes its LDS to its slice's partial.
//               One body with k17_edge: k_rank_edge_t over K11Space / K17Space
//   k11_node    per node row: FIRST: A from the workgroups' seed sums, W from the partials, p, R and r = p; else r = base + the
//               partials of the edge pass before it.  Then, unless LAST, m, t = m / W and base = R + m - t * W for the next
//               iteration; LAST: the window's sg_node_rank row.
//   k11_keys    K7's key pass over the rank rows: min(rank >> 24, 2^32 - 1) where share >= min_share; then K7's passes and
//               k_gather_sel (sg_kernels.h) as the node selection (k_gather: sg_window_rank with an index).
#pragma once

#define K11_THREADS 256           // k11_prep, k11_node
#define K11_EDGE_THREADS 1024     // k11_edge, k17_edge
#define K11_NR 16384              // nodes per range: 16384 x 8 B = 128 KiB of LDS
#define K11_Q 4                   // rows per thread and trip of k11_edge, k17_edge
#define K11_MAX_WGS 1024          // k11_prep's grid at most (k11_node sums one seed sum per workgroup)
#define K11_M_LOG2 56             // M = 2^56

static_assert(sizeof(sg_node_rank) == 16 && sizeof(sg_rank_params) == 24, "sg_node_rank / sg_rank_params layout");

struct RankArgs {
    NodesArgs nd;                 // K9's part: rows, ctr, max_edges, mk, ml, mob, ncap (k9_node, k9_used, k9_rows_of)
    const sg_node_out* nodes;     // the window's node rows
    const u64* count;             // their count
    u32 slices, prep_wgs;         // row slices of k11_edge; workgroups of k11_prep
    u32 damping, seed;            // D in 1..255; SG_RANK_SEED_*
    float seed_min;
    u32* src; u32* dst; u32* w;   // [max_edges] per row: node keys and weight
    u64* W; u64* R; u64* base; u64* t;   // [ncap] by node key
    u64* part;                    // [ranges][slices][K11_NR] per-slice partials
    u64* seed_sum;                // [K11_MAX_WGS] per workgroup of k11_prep
    sg_node_rank* out;            // [ncap] this window's rank rows
};

__device__ __forceinline__ u32 k11_q16(float s) { return s > 0.0f ? (s >= 1.0f ? 65536u : (u32)(s * 65536.0f)) : 0u; }
// the seed of a node row (K11) or a workload row (K17) under SG_RANK_SEED_* seed
__device__ __forceinline__ u64 k11_seed_of(u32 seed, float seed_min, float score) {
    if (seed == SG_RANK_SEED_UNIFORM) return 1ull;
    return score >= seed_min ? (u64)k11_q16(score) : 0ull;
}

// (k11_prep stays K11's own: K17 needs pos before its rows can be prepared and splits the work into k17_pos + k17_prep)
__global__ __launch_bounds__(K11_THREADS) void k11_prep(RankArgs a) {
    __shared__ u64 ssum;
    const u32 t = threadIdx.x;
    if (t == 0) ssum = 0;
    __syncthreads();
    const u64 E = k9_rows_of(a.nd), stride = (u64)gridDim.x * K11_THREADS, g0 = (u64)blockIdx.x * K11_THREADS + t;
    for (u64 j = g0; j < E; j += stride) {
        const u64* r = reinterpret_cast<const u64*>(a.nd.rows + j);  // word 3: from | to << 32; word 5 low: the score (sg_k5.h)
        const u64 ft = r[3];
        const float sc = __uint_as_float((u32)r[5]);
        u32 s = k9_node(a.nd, (u32)ft), d = k9_node(a.nd, (u32)(ft >> 32)), w = 1u + k11_q16(sc);
        if (s == SG_NONE || d == SG_NONE) { s = 0; d = 0; w = 0; }    // (a ref beyond the id spaces has no node row: the row carries nothing)
        a.src[j] = s; a.dst[j] = d; a.w[j] = w;
    }
    const u64 N = sg_nodes_of(a.count, a.nd.ncap);
    u64 sum = 0;
    for (u64 v = g0; v < N; v += stride) sum += k11_seed_of(a.seed, a.seed_min, a.nodes[v].score);
    if (sum) atomicAdd(&ssum, sum);
    __syncthreads();
    if (t == 0) a.seed_sum[blockIdx.x] = ssum;
}

// The edge pass of K11 and of K17 (sg_group_rank.h) is one body over a space policy: the nodes per range, the edge count, which
// node indices [n0, n0 + nr) workgroup range rg accumulates (false: it has nothing to do, and the node pass reads no partial of
// it), and whether an edge of weight 0 skips the load of t[src].  The weights' type comes with the space's Args (u32 here, u64 in K17).
struct K11Space {
    typedef RankArgs Args;
    static constexpr u32 NR = K11_NR;
    static constexpr bool SKIP_T_OF_ZERO_W = false;                  // (k11_prep gives a row that carries nothing src = 0, a valid key)
    static __device__ __forceinline__ u64 edges(const RankArgs& a) { return k9_rows_of(a.nd); }
    static __device__ __forceinline__ bool range(const RankArgs& a, u32 rg, u32& n0, u32& nr) {
        n0 = rg * K11_NR;
        if (n0 >= a.nd.ncap) return false;
        nr = a.nd.ncap - n0 < K11_NR ? a.nd.ncap - n0 : K11_NR;
        return k9_range_used(k9_used(a.nd), n0, n0 + nr);            // (no node row has a key in an unused range)
    }
};

template <class SP, bool BY_SRC>
__device__ __forceinline__ void k_rank_edge_t(const typename SP::Args& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* acc = reinterpret_cast<u64*>(smem);
    const u32 S = a.slices, g = blockIdx.x, t = threadIdx.x;
    const u32 rg = g / S, sl = g % S;
    u32 n0, nr;
    if (!SP::range(a, rg, n0, nr)) return;                           // (uniform)
    for (u32 i = t; i < nr; i += K11_EDGE_THREADS) acc[i] = 0;
    __syncthreads();
    const u64 E = SP::edges(a);
    const u64 per = (E + S - 1) / S, p0 = (u64)sl * per < E ? (u64)sl * per : E, p1 = p0 + per < E ? p0 + per : E;
    const u32* key = BY_SRC ? a.src : a.dst;
    for (u64 pb = p0 + t; pb < p1; pb += (u64)K11_EDGE_THREADS * K11_Q) {
        u32 k[K11_Q];
#pragma unroll
        for (int q = 0; q < K11_Q; q++) { const u64 p = pb + (u64)q * K11_EDGE_THREADS; k[q] = p < p1 ? key[p] - n0 : 0xFFFFFFFFu; }
#pragma unroll
        for (int q = 0; q < K11_Q; q++) if (k[q] < nr) {
            const u64 p = pb + (u64)q * K11_EDGE_THREADS;
            const u64 w = a.w[p];
            u64 x = w;                                               // (edges are sorted by source: t[src] is a cached, mostly uniform load)
            if constexpr (!BY_SRC) x = SP::SKIP_T_OF_ZERO_W && !w ? 0ull : a.t[a.src[p]] * w;
            if (x) atomicAdd(&acc[k[q]], x);
        }
    }
    __syncthreads();
    u64* out = a.part + ((size_t)rg * S + sl) * SP::NR;
    for (u32 i = t; i < nr; i += K11_EDGE_THREADS) out[i] = acc[i];
}
template <bool BY_SRC>
__global__ __launch_bounds__(K11_EDGE_THREADS) void k11_edge(RankArgs a) { k_rank_edge_t<K11Space, BY_SRC>(a); }

// the slices' partials of node key v summed
__device__ __forceinline__ u64 k11_part_sum(const RankArgs& a, u32 v) {
    const u32 rg = v / K11_NR, i = v - rg * K11_NR, S = a.slices;
    const u64* p = a.part + (size_t)rg * S * K11_NR + i;
    u64 s = 0;
    for (u32 sl = 0; sl < S; sl++) s += p[(size_t)sl * K11_NR];
    return s;
}

// (k11_node stays K11's own: it goes through k9_node, one thread a node row; k17_node splits a row's slices over eight threads)
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(K11_THREADS) void k11_node(RankArgs a) {
    __shared__ u64 sA;
    const u32 t = threadIdx.x;
    const u64 N = sg_nodes_of(a.count, a.nd.ncap);
    u64 A = 0;
    if (FIRST) {
        if (t == 0) sA = 0;
        __syncthreads();
        u64 s = 0;
        for (u32 i = t; i < a.prep_wgs; i += K11_THREADS) s += a.seed_sum[i];
        if (s) atomicAdd(&sA, s);
        __syncthreads();
        A = sA;
    }
    const u64 D = a.damping, M = 1ull << K11_M_LOG2;
    for (u64 i = (u64)blockIdx.x * K11_THREADS + t; i < N; i += (u64)gridDim.x * K11_THREADS) {
        const sg_node_out* nrow = a.nodes + i;
        const u32 ref = nrow->ref, v = k9_node(a.nd, ref);
        if (v == SG_NONE) continue;                                   // (cannot be: K9 made the row from such a key)
        u64 r, W = 0, R = 0;
        if (FIRST) {
            const u64 av = A ? k11_seed_of(a.seed, a.seed_min, nrow->score) : 1ull;   // A == 0: the uniform seed
            const u64 p = av * (M / (A ? A : N));
            W = k11_part_sum(a, v);
            R = (p >> 8) * (256 - D);
            a.W[v] = W; a.R[v] = R;
            r = p;
        } else {
            r = a.base[v] + k11_part_sum(a, v);
        }
        if (LAST) {
            sg_node_rank o;
            o.rank = r; o.ref = ref; o.share = (float)((double)r * 0x1p-56);
            a.out[i] = o;
        } else {
            if (!FIRST) { W = a.W[v]; R = a.R[v]; }
            const u64 m = (r >> 8) * D, tt = W ? m / W : 0ull;
            a.t[v] = tt;
            a.base[v] = R + (m - tt * W);
        }
    }
}

// k7_keys over rank rows (k10_keys' shape): key = min(rank >> 24, 2^32 - 1) where share >= min_share, else 0.  Workgroup 0 copies
// the node count to ctr[C_N_EDGES], where K7's later passes read it.
__global__ __launch_bounds__(K7_THREADS) void k11_keys(SelArgs a, const sg_node_rank* rank, const u64* count, u64* ctr) {
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
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        const sg_node_rank r = rank[i];
        const u64 k = r.rank >> 24;
        const u32 key = r.share >= a.min_score ? (k > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)k) : 0u;
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}
