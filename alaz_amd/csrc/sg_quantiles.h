// sg_quantiles.h — K20: latency histograms and percentiles per node row, group edge and workload row (include/servicegraph.h,
// "latency percentiles").  Included after sg_group_track.h: it reuses K9's node key (k9_node), K16's group key (k16_gk) and the
// counts' helpers (sg_nodes_of, k9_rows_of, k16_edges_of) as they are; every kernel here is its own.
//
// The source is always the window's row histograms in row order (Dev::hist_csr, 16 u32 bins a row): the workload rows fold the ROWS,
// along perm, not the group-edge histograms — the same policy as the group edges' fold, and the three spaces stay independent of
// each other.  Work is in ROW-INDEX space (node-row position, group-edge index, workload-row position), so every table is dense:
//
//   k20_pos_nodes / k20_pos_groups   per node row / workload row v: pos[key(ref_v)] = v.  Only the window's keys are written and
//                 only those are read: nothing is zeroed between windows
//   k20_tgt_nodes / k20_tgt_groups / k20_tgt_group_nodes   per source position p: the target position(s) as 4-byte words — row p's
//                 from and to node rows; the group edge of row perm[p]; that group edge's from and to workload rows
//   k20_fold      ONE body for every side.  Workgroup (range, slice): K20_NR targets x 16 u64 bins in LDS (64 KiB: two workgroups a
//                 CU).  It scans its slice of the 4-byte targets, K20_C positions a trip, and loads the 64-byte histogram (through
//                 perm where the side has one) only of positions whose target is in its range; non-zero bins are added with LDS
//                 integer atomics, and the LDS goes to the (range, slice) partial.  On a side whose targets are non-decreasing
//                 along the scan (the out sides, the group edges) a range scans only its own span of positions, found by two
//                 binary searches, cut into the slices.  A hub is spread over the slices and the lanes; device memory sees no
//                 atomic at all.  Integer adds only: the partials' sum does not depend on the split
//   k20_finish    16 lanes an entity and side: lane b sums bin b over the slices, writes hist[entity][side][b], the 16 lanes scan the
//                 bins with shuffles and lane j < n_q finds quantile j from the cumulative counts and the entity's own max_ns
//
// A bin of an entity is a sum of at most 2^32 u32 bins: below 2^64.  The partial of a slice sums at most its positions: no carry is
// lost anywhere, and the fold has one correct value.
#pragma once

#define K20_THREADS 256           // k20_pos_*, k20_tgt_*, k20_finish
#define K20_FOLD_THREADS 512      // k20_fold
#define K20_C K20_FOLD_THREADS    // source positions per workgroup trip: one a thread
#define K20_NR 512                // targets per range: 512 x 16 bins x 8 B = 64 KiB of LDS
#define K20_MAX_WGS 1024          // grid-stride grids at most
#define K20_ENT (K20_THREADS / SG_HIST_BINS)   // entities per workgroup and round of k20_finish

static_assert(SG_HIST_BINS == 16 && SG_Q_MAX <= SG_HIST_BINS, "k20_fold / k20_finish: 16 bins, a quantile a lane of the entity's 16");

__device__ __forceinline__ u32 k20_clip(u32 t, u64 N) { return t < N ? t : SG_NONE; }

__global__ __launch_bounds__(K20_THREADS) void k20_pos_nodes(NodesArgs nd, const sg_node_out* nodes, const u64* count, u32* pos) {
    const u64 N = sg_nodes_of(count, nd.ncap);
    for (u64 v = (u64)blockIdx.x * K20_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K20_THREADS) {
        const u32 k = k9_node(nd, nodes[v].ref);
        if (k != SG_NONE && k < nd.ncap) pos[k] = (u32)v;            // (cannot fail: K9 made the row from such a key)
    }
}
// per row j: the node rows of its endpoints
__global__ __launch_bounds__(K20_THREADS) void k20_tgt_nodes(NodesArgs nd, const u64* count, const u32* pos, u32* tout, u32* tin) {
    const u64 E = k9_rows_of(nd), N = sg_nodes_of(count, nd.ncap);
    for (u64 j = (u64)blockIdx.x * K20_THREADS + threadIdx.x; j < E; j += (u64)gridDim.x * K20_THREADS) {
        const u64 ft = reinterpret_cast<const u64*>(nd.rows + j)[3];   // from_ref | to_ref << 32
        const u32 fk = k9_node(nd, (u32)ft), tk = k9_node(nd, (u32)(ft >> 32));
        tout[j] = fk != SG_NONE && fk < nd.ncap ? k20_clip(pos[fk], N) : SG_NONE;
        tin[j] = tk != SG_NONE && tk < nd.ncap ? k20_clip(pos[tk], N) : SG_NONE;
    }
}
__global__ __launch_bounds__(K20_THREADS) void k20_pos_groups(GroupNodesArgs g, const sg_node_out* nodes, const u64* count, u32* pos) {
    const u64 N = sg_nodes_of(count, g.nc);
    for (u64 v = (u64)blockIdx.x * K20_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K20_THREADS) {
        const u32 k = k16_gk(g, nodes[v].ref);
        if (k != SG_NONE && k < g.gk) pos[k] = (u32)v;               // (cannot fail: K16 made the row from such a key)
    }
}
// the group edge of the row at position p of perm (SG_NONE: a stray index, no window has one)
__device__ __forceinline__ u32 k20_group_at(const u32* perm, const u32* row_group, u64 p, u64 E, u64 G) {
    const u32 j = perm[p];
    if (j >= E) return SG_NONE;
    const u32 g = row_group[j];
    return g < G ? g : SG_NONE;
}
__global__ __launch_bounds__(K20_THREADS) void k20_tgt_groups(GroupNodesArgs g, const u32* perm, const u32* row_group, u32* tgt) {
    const u64 E = k9_rows_of(g.nd), G = k16_edges_of(g);
    for (u64 p = (u64)blockIdx.x * K20_THREADS + threadIdx.x; p < E; p += (u64)gridDim.x * K20_THREADS)
        tgt[p] = k20_group_at(perm, row_group, p, E, G);
}
// per position p of perm: the workload rows of the endpoints of the row's group edge
__global__ __launch_bounds__(K20_THREADS) void k20_tgt_group_nodes(GroupNodesArgs g, const u32* perm, const u32* row_group, const u64* count,
                                                                    const u32* pos, u32* tout, u32* tin) {
    const u64 E = k9_rows_of(g.nd), G = k16_edges_of(g), N = sg_nodes_of(count, g.nc);
    for (u64 p = (u64)blockIdx.x * K20_THREADS + threadIdx.x; p < E; p += (u64)gridDim.x * K20_THREADS) {
        const u32 ge = k20_group_at(perm, row_group, p, E, G);
        u32 o = SG_NONE, i = SG_NONE;
        if (ge != SG_NONE) {
            const u64 ft = reinterpret_cast<const u64*>(g.groups + ge)[6];   // from_ref | to_ref << 32 (byte 48)
            const u32 fk = k16_gk(g, (u32)ft), tk = k16_gk(g, (u32)(ft >> 32));
            if (fk != SG_NONE && fk < g.gk) o = k20_clip(pos[fk], N);
            if (tk != SG_NONE && tk < g.gk) i = k20_clip(pos[tk], N);
        }
        tout[p] = o; tin[p] = i;
    }
}

struct QuantFoldArgs {
    const u32* bins;              // the window's row histograms, row order (Dev::hist_csr)
    const u32* perm;              // the row at a position (nullptr: position = row)
    const u32* tgt;               // [max_edges] the target of a position (SG_NONE: none)
    const u64* ctr;               // the window's counters: E = ctr[C_N_EDGES]
    u64 max_edges;
    const u64* tcount; u32 tcap;  // the targets of the window, their capacity
    u32 slices, sorted;           // slices a range; sorted: tgt is non-decreasing along the positions
    u64* part;                    // [ranges][slices][K20_NR][16] partials
};
// the first position in [0, E) whose target is >= x (targets non-decreasing)
__device__ __forceinline__ u64 k20_lower(const u32* tgt, u64 E, u64 x) {
    u64 lo = 0, hi = E;
    while (lo < hi) { const u64 m = lo + ((hi - lo) >> 1); if ((u64)tgt[m] < x) lo = m + 1; else hi = m; }
    return lo;
}
// bin b of target i sits at word ((b + i) & 15) of the target's 16: equal bins of different targets fall on different LDS banks
__device__ __forceinline__ u32 k20_word(u32 i, u32 b) { return i * SG_HIST_BINS + ((b + i) & (SG_HIST_BINS - 1)); }

__global__ __launch_bounds__(K20_FOLD_THREADS) void k20_fold(QuantFoldArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* acc = reinterpret_cast<u64*>(smem);
    const u32 S = a.slices, rg = blockIdx.x / S, sl = blockIdx.x % S, t = threadIdx.x;
    const u64 N = sg_nodes_of(a.tcount, a.tcap), first = (u64)rg * K20_NR;
    if (first >= N) return;                                          // (uniform; k20_finish reads no partial of such a range)
    const u32 n0 = (u32)first, nr = N - first < K20_NR ? (u32)(N - first) : K20_NR;
    for (u32 i = t; i < nr * SG_HIST_BINS; i += K20_FOLD_THREADS) acc[i] = 0;
    u64 E = a.ctr[C_N_EDGES]; E = E < a.max_edges ? E : a.max_edges;
    u64 q0 = 0, q1 = E;
    if (a.sorted) { q0 = k20_lower(a.tgt, E, first); q1 = k20_lower(a.tgt, E, first + nr); }   // (every thread the same ~2 x 20 loads)
    const u64 per = (q1 - q0 + S - 1) / S;
    const u64 p0 = q0 + (u64)sl * per < q1 ? q0 + (u64)sl * per : q1, p1 = p0 + per < q1 ? p0 + per : q1;
    __syncthreads();
    for (u64 p = p0 + t; p < p1; p += K20_C) {
        const u32 to = a.tgt[p] - n0;
        if (to >= nr) continue;
        const u64 j = a.perm ? (u64)a.perm[p] : p;
        if (j >= E) continue;
        const uint4* hp = reinterpret_cast<const uint4*>(a.bins + j * SG_HIST_BINS);
        const uint4 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3];
        const u32 hb[SG_HIST_BINS] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w, h3.x, h3.y, h3.z, h3.w};
#pragma unroll
        for (u32 b = 0; b < SG_HIST_BINS; b++) if (hb[b]) atomicAdd(&acc[k20_word(to, b)], (u64)hb[b]);
    }
    __syncthreads();
    u64* out = a.part + ((size_t)rg * S + sl) * K20_NR * SG_HIST_BINS;
    for (u32 i = t; i < nr * SG_HIST_BINS; i += K20_FOLD_THREADS) out[i] = acc[k20_word(i / SG_HIST_BINS, i % SG_HIST_BINS)];
}

struct QuantFinishArgs {
    const u64* part; u32 slices;
    const u64* tcount; u32 tcap;
    const unsigned char* ent; u32 stride, max_off;   // the entities' rows: max_ns of entity v at ent + v * stride + max_off
    u64* hist;                    // [entities][sides][16]
    u32* quant;                   // [entities][sides][SG_Q_MAX]
    u32 sides, side, n_q;
    u64 qm[2];                    // the per-mille, 16 bits each
};
// the value lane `src` of the wave holds (every lane of the wave calls it): written out over the bpermute, not __shfl with a width —
// a second width among the translation unit's calls changed how the existing kernels' __shfl calls compile
__device__ __forceinline__ u64 k20_lane_get(u64 v, u32 src) {
    const u32 lo = (u32)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(u32)v);
    const u32 hi = (u32)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}
// Q(B, max_ns, qm) of include/servicegraph.h from the bins' cumulative counts, held a bin a lane in the entity's 16 lanes
__device__ __forceinline__ u32 k20_quantile(u64 cum, u32 base, u64 total, u64 max_ns, u32 qm) {
    u64 rank = (total / 1000ull) * qm + ((total % 1000ull) * qm + 999ull) / 1000ull;
    rank = rank ? rank : 1ull;
    u32 bq = SG_HIST_BINS - 1; bool found = false;
#pragma unroll
    for (u32 b = 0; b < SG_HIST_BINS; b++) {
        const u64 c = k20_lane_get(cum, base + b);
        if (!found && c >= rank) { bq = b; found = true; }
    }
    u64 e = bq == SG_HIST_BINS - 1 ? max_ns : (1ull << (17 + bq));
    e = e > max_ns ? max_ns : e;
    e /= 1000ull;
    return total ? (e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)e) : 0u;
}
__global__ __launch_bounds__(K20_THREADS) void k20_finish(QuantFinishArgs a) {
    const u32 b = threadIdx.x % SG_HIST_BINS, g = threadIdx.x / SG_HIST_BINS, S = a.slices;
    const u32 lane = threadIdx.x & 63u, base = lane - b;             // (a wave is 64 consecutive threads: four entities)
    const u64 N = sg_nodes_of(a.tcount, a.tcap);
    const u32 qm = (u32)((b < 4 ? a.qm[0] >> (16 * b) : a.qm[1] >> (16 * (b & 3u))) & 0xFFFFull);
    for (u64 v0 = (u64)blockIdx.x * K20_ENT; v0 < N; v0 += (u64)gridDim.x * K20_ENT) {   // (uniform: every thread takes every round)
        const bool live = v0 + g < N;
        const u64 v = live ? v0 + g : N - 1;
        const u64 rg = v / K20_NR, i = v - rg * K20_NR;
        const u64* p = a.part + (rg * S * K20_NR + i) * SG_HIST_BINS + b;
        u64 s = 0;
        for (u32 sl = 0; sl < S; sl++) s += p[(size_t)sl * K20_NR * SG_HIST_BINS];
        u64 cum = s;
#pragma unroll
        for (u32 d = 1; d < SG_HIST_BINS; d <<= 1) { const u64 o = k20_lane_get(cum, b >= d ? lane - d : lane); if (b >= d) cum += o; }
        const u64 total = k20_lane_get(cum, base + SG_HIST_BINS - 1);
        const u64 max_ns = *reinterpret_cast<const u64*>(a.ent + v * a.stride + a.max_off);
        const u32 q = k20_quantile(cum, base, total, max_ns, qm);
        if (!live) continue;
        const u64 o = v * a.sides + a.side;
        a.hist[o * SG_HIST_BINS + b] = s;
        if (b < a.n_q) a.quant[o * SG_Q_MAX + b] = q;
    }
}
