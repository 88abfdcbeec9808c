// sg_k3.h — K3 node statistics and features, the window reset
// Part of the kernel translation unit: included by sg_kernels.h (which holds the shared helpers), in this order.
#pragma once

// ---- in-statistics: per destination node, reduce over its in-edges --------------------------------
// No device-scope atomics (they top out at ~22 G/s chip-wide: the hashed-LDS + atomic-flush version of round 1 spent
// 175 us on C3's 1 M edges = 2.4 % of the HBM roofline).  Two launches instead:
//   k3_in_part   grid = node ranges x edge slices.  Workgroup (r, s) owns the K3_IN_NR nodes of range r in node-indexed
//                LDS arrays, scans slice s of the CSR destination column (coalesced u32 reads, L2-resident across the
//                ranges) and folds the accumulators of the edges that point into its range with LDS atomics; then it
//                writes its arrays to the partial buffer with plain coalesced stores.
//   k3_in_reduce one thread per (node, word): sums (max for the last word) the slices' partials into st_sum / st_max.
// Exact (integer sums and max are order-free) and deterministic.
// The window's open connections (SG_EV_ALIVE, f-2) are marked here too: every record's edge exists in
// the CSR (K1 created it with count 0 if it carried no request); a binary search in the sorted row
// finds it.  Costs one scalar load when the window has none.
__device__ __forceinline__ void alive_mark(const Dev& d, u32 g, u32 G, u32 t) {
    const u64 n_all = d.ctr[C_ALIVE_N];
    if (n_all == 0) return;
    const u32 n = (u32)(n_all < d.alive_cap ? n_all : d.alive_cap);
    const u32 nk = (u32)d.ctr[C_N_KNOWN], nl = (u32)d.ctr[C_N_LABELS], nob = (u32)d.ctr[C_N_OBIP];
    for (u32 i = g * 1024 + t; i < n; i += G * 1024) {
        const u64 key = d.alive_keys[i];
        const u32 f = dense_of(d, (u32)(key >> 32), nk, nl, nob), to = dense_of(d, (u32)key, nk, nl, nob);
        bool ok = f != SG_NONE && to != SG_NONE;
        if (ok) {
            u32 lo = d.rowptr[f], hi = d.rowptr[f + 1];
            if ((u64)hi > d.max_edges) hi = (u32)d.max_edges;
            const u32 end = hi;
            while (lo < hi) { const u32 m = (lo + hi) >> 1; if (d.col[m] < to) lo = m + 1; else hi = m; }
            ok = lo < end && d.col[lo] == to;
            if (ok) {
                atomicAdd(&d.alive_csr[lo], 1u);
                atomicAdd(&d.st_sum[(size_t)f * SG_NODE_STAT_SUM_WORDS + ST_OUT_ALIVE], 1ull);
                atomicAdd(&d.st_sum[(size_t)to * SG_NODE_STAT_SUM_WORDS + ST_IN_ALIVE], 1ull);
            }
        }
        if (!ok) atomicAdd(&d.ctr[C_ALIVE_DROP], 1ull);
    }
}

// fin (the one-call pipelines, whose node features sum the slices' partials themselves — k3_node_features — so that k3_in_reduce is not
// launched): the launch's LAST fin workgroups do what k3_in_reduce's last ones do in the staged pipelines — finish the rows behind
// kw_compact (degree, mean / deviation, hub work items), or the block-sorted rows of an engine without the kept state.
// FORM (Plan::k3_in_form): 0 = the scan as it was written first — the accumulator loads under their range test, the next destinations
// under their bounds test: as compiled, each of the sixteen is a block of its own that waits for its load, so a trip is sixteen dependent
// round trips.  1 = every load of a trip is unconditional and issued before the first wait: an index past the slice is clamped to its
// last position and the value replaced by a select; a lane whose destination lies outside the range loads the accumulators of the
// slice's FIRST position instead of its own (one line for all such lanes of a wave — four of five at C3 — so the fetched bytes stay what
// they were) and drops them.  Same partials: the LDS atomics stay under the range test.
template <int FORM>
__global__ __launch_bounds__(1024) void k3_in_part(Dev d, u32 S, u32 fin) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 E = (u32)d.ctr[C_N_EDGES], N = (u32)d.ctr[C_N_NODES];
    const u32 G = gridDim.x - fin, g = blockIdx.x, t = threadIdx.x;
    if (g >= G) {
        if (d.warm) kw_finish_rows(d, (g - G) * 1024 + t, fin * 1024);
        else if (g == gridDim.x - 1) k2_split_finish(d, t, 1024);
        return;
    }
    SG_STAMP(d, 3, 0);
    // a delta window's kw_compact (the launch before this one) has written the kept CSR, grown by the window's new edges, to the other
    // buffer: flip (nothing in this launch reads the kept state; the next window's pass B and kw_compact do)
    if (g == 0 && t == 0 && d.warm && !d.ctr[C_COLD] && d.ctr[C_DELTA_N]) {
        d.ctr[C_KEPT_E] += (u64)d.dc_rowptr[d.max_known + d.max_labels];
        d.ctr[C_KEPT_BUF] ^= 1ull;                                    // (C_DELTA_N stays until the window reset; the window's reader takes kw_compact's copy, C_LAST_DELTA)
    }
    alive_mark(d, g, G, t);
    const u32 r = g / S, sl = g % S, n0 = r * K3_IN_NR;
    if (n0 >= N) return;
    const u32 nr = N - n0 < K3_IN_NR ? N - n0 : K3_IN_NR;
    u64* acc = reinterpret_cast<u64*>(smem);                         // [nr][6]: deg, cnt, err, sum, ssq, max
    for (u32 i = t; i < nr * 6; i += 1024) acc[i] = 0;
    __syncthreads();
    SG_STAMP(d, 3, 1);
    const u32 per = (E + S - 1) / S, p0 = sl * per < E ? sl * per : E, p1 = p0 + per < E ? p0 + per : E;
    // Eight edges per thread and trip; the destinations of the NEXT trip are fetched behind this trip's accumulator loads, so a
    // trip costs one round trip, not two (a slice of C3 is 31 k edges: four trips; at four edges per trip and no lookahead the
    // sixteen dependent round trips were most of this kernel's 22 us).
    constexpr int K3Q = 8;
    u32 nxt[K3Q];
    if constexpr (FORM == 0) {
#pragma unroll
        for (int q = 0; q < K3Q; q++) { const u32 p = p0 + t + q * 1024; nxt[q] = p < p1 ? d.col[p] - n0 : 0xFFFFFFFFu; }
        for (u32 pb = p0 + t; pb < p1; pb += 1024 * K3Q) {
            u32 to[K3Q];
            ulonglong2 x[K3Q], y[K3Q];
#pragma unroll
            for (int q = 0; q < K3Q; q++) {
                to[q] = nxt[q];
                if (to[q] < nr) { const ulonglong2* a = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)(pb + q * 1024) * 4); x[q] = a[0]; y[q] = a[1]; }
            }
#pragma unroll
            for (int q = 0; q < K3Q; q++) { const u32 p = pb + 1024 * K3Q + q * 1024; nxt[q] = p < p1 ? d.col[p] - n0 : 0xFFFFFFFFu; }
#pragma unroll
            for (int q = 0; q < K3Q; q++) if (to[q] < nr) {
                u64* o = acc + (size_t)to[q] * 6;
                atomicAdd(&o[0], 1ull); atomicAdd(&o[1], x[q].x & 0xFFFFFFFFull); if (x[q].x >> 32) atomicAdd(&o[2], x[q].x >> 32);
                atomicAdd(&o[3], x[q].y); atomicAdd(&o[4], y[q].y); atomicMax(&o[5], y[q].x);
            }
        }
    } else {
        const u32 last = p1 - 1;                                     // (read where the slice is not empty only)
        if (p0 < p1) {
            u32 raw[K3Q];
#pragma unroll
            for (int q = 0; q < K3Q; q++) { const u32 p = p0 + t + q * 1024; raw[q] = d.col[p < p1 ? p : last]; }
#pragma unroll
            for (int q = 0; q < K3Q; q++) nxt[q] = p0 + t + q * 1024 < p1 ? raw[q] - n0 : 0xFFFFFFFFu;
        } else {
#pragma unroll
            for (int q = 0; q < K3Q; q++) nxt[q] = 0xFFFFFFFFu;
        }
        for (u32 pb = p0 + t; pb < p1; pb += 1024 * K3Q) {
            u32 to[K3Q], raw[K3Q];
            ulonglong2 x[K3Q], y[K3Q];
#pragma unroll
            for (int q = 0; q < K3Q; q++) { to[q] = nxt[q]; const u32 p = pb + 1024 * K3Q + q * 1024; raw[q] = d.col[p < p1 ? p : last]; }
#pragma unroll
            for (int q = 0; q < K3Q; q++) {
                const ulonglong2* a = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)(to[q] < nr ? pb + q * 1024 : p0) * 4);
                x[q] = a[0]; y[q] = a[1];
            }
            // the trip's one wait: nothing above it may sink below (the compiler would move each pair into the block of its atomics)
            asm volatile("" : "+v"(x[0].x), "+v"(x[0].y), "+v"(y[0].x), "+v"(y[0].y) : : "memory");
#pragma unroll
            for (int q = 1; q < K3Q; q++) asm volatile("" : "+v"(x[q].x), "+v"(x[q].y), "+v"(y[q].x), "+v"(y[q].y));
#pragma unroll
            for (int q = 0; q < K3Q; q++) nxt[q] = pb + 1024 * K3Q + q * 1024 < p1 ? raw[q] - n0 : 0xFFFFFFFFu;
#pragma unroll
            for (int q = 0; q < K3Q; q++) if (to[q] < nr) {
                u64* o = acc + (size_t)to[q] * 6;
                atomicAdd(&o[0], 1ull); atomicAdd(&o[1], x[q].x & 0xFFFFFFFFull); if (x[q].x >> 32) atomicAdd(&o[2], x[q].x >> 32);
                atomicAdd(&o[3], x[q].y); atomicAdd(&o[4], y[q].y); atomicMax(&o[5], y[q].x);
            }
        }
    }
    SG_STAMP(d, 3, 2);
    __syncthreads();
    SG_STAMP(d, 3, 3);
    u64* out = d.in_part + ((size_t)r * S + sl) * K3_IN_NR * 6;
    for (u32 i = t; i < nr * 6; i += 1024) out[i] = acc[i];
    SG_STAMP(d, 3, 4);
}
__global__ __launch_bounds__(256) void k3_in_reduce(Dev d, u32 S, u32 fin) {
    const u32 N = (u32)d.ctr[C_N_NODES];
    // the out-statistics of the rows the row sort took block by block: the launch's LAST workgroup, and nothing else there (three
    // dependent round trips — in front of the reduction they were on the path of the threads that ran both)
    // (an engine that keeps state: the last `fin` workgroups finish EVERY row behind kw_compact instead — degree, mean / deviation, hub work items)
    if (blockIdx.x >= gridDim.x - fin) {
        if (d.warm) kw_finish_rows(d, (blockIdx.x - (gridDim.x - fin)) * 256 + threadIdx.x, fin * 256);
        else if (blockIdx.x == gridDim.x - 1) k2_split_finish(d, threadIdx.x, 256);
        return;
    }
    const u32 GW = gridDim.x - fin;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < (u64)N * 6; i += (u64)GW * 256) {
        const u32 v = (u32)(i / 6), k = (u32)(i % 6), r = v / K3_IN_NR;
        const u64* p = d.in_part + ((size_t)r * S * K3_IN_NR + (v - r * K3_IN_NR)) * 6 + k;
        const size_t st = (size_t)K3_IN_NR * 6;
        u64 a = 0;
        u32 sl = 0;
        // (measured: all 32 slices in one batch of loads instead of four batches of eight — 10.1 -> 12.1 us on one kind of box)
        if (k == 5) {
            for (; sl + 8 <= S; sl += 8) {                           // eight independent loads in flight
                u64 x[8];
#pragma unroll
                for (int q = 0; q < 8; q++) x[q] = p[(size_t)(sl + q) * st];
#pragma unroll
                for (int q = 0; q < 8; q++) a = x[q] > a ? x[q] : a;
            }
            for (; sl < S; sl++) { const u64 x = p[(size_t)sl * st]; a = x > a ? x : a; }
            d.st_max[(size_t)v * 2 + 1] = a;
        } else {
            for (; sl + 8 <= S; sl += 8) {
                u64 x[8];
#pragma unroll
                for (int q = 0; q < 8; q++) x[q] = p[(size_t)(sl + q) * st];
#pragma unroll
                for (int q = 0; q < 8; q++) a += x[q];
            }
            for (; sl < S; sl++) a += p[(size_t)sl * st];
            d.st_sum[(size_t)v * SG_NODE_STAT_SUM_WORDS + (k == 0 ? ST_IN_DEG : k == 1 ? ST_IN_CNT : k == 2 ? ST_IN_ERR : k == 3 ? ST_IN_SUM : ST_IN_SSQ)] = a;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K3  node_features: fp32 x_v from the integer node statistics.
// ------------------------------------------------------------------------------------------------
// Two lanes per node: lane 0 of the pair turns the out-side statistics into features, lane 1 the
// in-side ones (the fp64 log1p / sqrt chains are the whole cost of this kernel), then they swap.
// Workgroups [0, nb_nodes) do the nodes; the rest do the edge features (one thread per edge, edge_features()).
// S_in != 0 (the one-call pipelines): the in-side lane of a node sums the S_in slices' partials of k3_in_part itself (and leaves the sums in
// st_sum / st_max, where the staged pipelines' k3_in_reduce puts them) — one launch and a 24 MB round trip less per window.
// The seven values of one side of a node, by index — the one copy of the arithmetic, for both kernels below:
//   0 log1p(deg)  1 log1p(cnt)  2 log1p(mean / 1000)  3 err / cnt  4 log1p(max / 1e6)  5 log1p(std / 1000)  6 log1p(alive)
// node_feature_arg<K> is what log1p takes (every K but 3).  K is a template argument so that k3_node_features, which runs all seven,
// compiles to what it was; node_feature_at picks by a lane's own index and runs ONE log1p whatever the index (k3_node_features_lanes).
template <int K>
__device__ __forceinline__ double node_feature_arg(u64 dg, u64 c, u64 sm, u64 sq, u64 mx, u64 al) {
    static_assert(K >= 0 && K <= 6 && K != 3, "3 is a quotient, not a logarithm");
    if constexpr (K == 0) return (double)dg;
    else if constexpr (K == 1) return (double)c;
    else if constexpr (K == 2) return mean_us(sm, c) / 1000.0;
    else if constexpr (K == 4) return (double)mx / 1e6;
    else if constexpr (K == 5) return std_us(sm, sq, c) / 1000.0;
    else return (double)al;
}
template <int K>
__device__ __forceinline__ float node_feature_value(u64 dg, u64 c, u64 er, u64 sm, u64 sq, u64 mx, u64 al) {
    if constexpr (K == 3) return c ? (float)((double)er / (double)c) : 0.0f;
    else return (float)log1p(node_feature_arg<K>(dg, c, sm, sq, mx, al));
}
__device__ __forceinline__ float node_feature_at(u32 k, u64 dg, u64 c, u64 er, u64 sm, u64 sq, u64 mx, u64 al) {
    if (k == 3) return node_feature_value<3>(dg, c, er, sm, sq, mx, al);
    const double x = k == 0 ? node_feature_arg<0>(dg, c, sm, sq, mx, al) : k == 1 ? node_feature_arg<1>(dg, c, sm, sq, mx, al) :
                     k == 2 ? node_feature_arg<2>(dg, c, sm, sq, mx, al) : k == 4 ? node_feature_arg<4>(dg, c, sm, sq, mx, al) :
                     k == 5 ? node_feature_arg<5>(dg, c, sm, sq, mx, al) : node_feature_arg<6>(dg, c, sm, sq, mx, al);
    return (float)log1p(x);
}
__global__ __launch_bounds__(256) void k3_node_features(Dev d, u32 nb_nodes, u32 S_in) {
    if (blockIdx.x >= nb_nodes) {
        const u32 E = (u32)d.ctr[C_N_EDGES];
        for (u32 p = (blockIdx.x - nb_nodes) * 256 + threadIdx.x; p < E; p += (gridDim.x - nb_nodes) * 256) edge_features(d, p);
        return;
    }
    const u32 N = (u32)d.ctr[C_N_NODES], nk = (u32)d.ctr[C_N_KNOWN];
    const u32 side = threadIdx.x & 1u;
    for (u32 v0 = blockIdx.x * 128; v0 < N; v0 += nb_nodes * 128) {
        const u32 v = v0 + (threadIdx.x >> 1);
        const bool live = v < N;
        float a[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            u64* s = d.st_sum + (size_t)v * SG_NODE_STAT_SUM_WORDS;
            u64 dg, c, er, sm, sq, mx;
            if (S_in && side) {                                      // deg, cnt, err, sum, ssq, max of the node's in-edges: over the slices (integer: order-free)
                const u32 r = v / K3_IN_NR;
                const ulonglong2* p = reinterpret_cast<const ulonglong2*>(d.in_part + ((size_t)r * S_in * K3_IN_NR + (v - r * K3_IN_NR)) * 6);
                const size_t st = (size_t)K3_IN_NR * 3;              // (16-byte words per slice)
                dg = c = er = sm = sq = mx = 0;
                u32 sl = 0;
                for (; sl + 4 <= S_in; sl += 4) {                    // twelve independent loads in flight
                    ulonglong2 x[4][3];
#pragma unroll
                    for (int q = 0; q < 4; q++) { x[q][0] = p[(size_t)(sl + q) * st]; x[q][1] = p[(size_t)(sl + q) * st + 1]; x[q][2] = p[(size_t)(sl + q) * st + 2]; }
#pragma unroll
                    for (int q = 0; q < 4; q++) { dg += x[q][0].x; c += x[q][0].y; er += x[q][1].x; sm += x[q][1].y; sq += x[q][2].x; mx = x[q][2].y > mx ? x[q][2].y : mx; }
                }
                for (; sl < S_in; sl++) {
                    const ulonglong2 a0 = p[(size_t)sl * st], a1 = p[(size_t)sl * st + 1], a2 = p[(size_t)sl * st + 2];
                    dg += a0.x; c += a0.y; er += a1.x; sm += a1.y; sq += a2.x; mx = a2.y > mx ? a2.y : mx;
                }
                s[ST_IN_DEG] = dg; s[ST_IN_CNT] = c; s[ST_IN_ERR] = er; s[ST_IN_SUM] = sm; s[ST_IN_SSQ] = sq; d.st_max[(size_t)v * 2 + 1] = mx;
            } else {
                dg = s[ST_OUT_DEG + side]; c = s[ST_OUT_CNT + side]; er = s[ST_OUT_ERR + side]; sm = s[ST_OUT_SUM + side]; sq = s[ST_OUT_SSQ + side];
                mx = d.st_max[(size_t)v * 2 + side];
            }
            a[0] = node_feature_value<0>(dg, c, er, sm, sq, mx, 0);
            a[1] = node_feature_value<1>(dg, c, er, sm, sq, mx, 0);
            a[2] = node_feature_value<2>(dg, c, er, sm, sq, mx, 0);
            a[3] = node_feature_value<3>(dg, c, er, sm, sq, mx, 0);
            a[4] = node_feature_value<4>(dg, c, er, sm, sq, mx, 0);
            a[5] = node_feature_value<5>(dg, c, er, sm, sq, mx, 0);
            a[6] = node_feature_value<6>(dg, c, er, sm, sq, mx, s[ST_OUT_ALIVE + side]);
        }
        float b[7];
#pragma unroll
        for (int k = 0; k < 7; k++) b[k] = __shfl_xor(a[k], 1, 64);
        if (!live) continue;
        float4* o = reinterpret_cast<float4*>(d.x0 + (size_t)v * SG_F_IN);
        if (side == 0) {                                             // a = out side, b = in side
            const u32 kind = v < nk ? d.kind[v] : 0u;
            o[0] = make_float4(a[0], b[0], a[1], b[1]);
            o[1] = make_float4(a[2], b[2], a[3], b[3]);
            o[2] = make_float4(a[4], b[4], kind == SG_NODE_POD ? 1.0f : 0.0f, kind == SG_NODE_SERVICE ? 1.0f : 0.0f);
            o[3] = make_float4(kind == 0 ? 1.0f : 0.0f, a[5], b[5], 1.0f);
        } else {                                                     // a = in side, b = out side
            o[4] = make_float4(b[6], a[6], 0.0f, 0.0f);
#pragma unroll
            for (int q = 5; q < (int)SG_F_IN / 4; q++) o[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {                       // the alive list is consumed (k3_in_stats): report and re-arm
        const u64 n = d.ctr[C_ALIVE_N];
        d.ctr[C_ALIVE_SEEN] = n;
        d.ctr[C_ALIVE_DROPPED] = d.ctr[C_ALIVE_DROP] + (n > d.alive_cap ? n - d.alive_cap : 0);
        d.ctr[C_ALIVE_N] = 0; d.ctr[C_ALIVE_DROP] = 0;
    }
}

// The node-only launch (Plan::k3_feat_lanes; the score kernel computes the edge features: Plan::k5_efeat) with EIGHT lanes per node, 32
// nodes per workgroup.  The in-side sums: lane j takes slices j, j + 8, ... — every load unconditional (slice index clamped, value
// dropped by a select) and a batch of them in flight at once, so the partials cost one round trip, not S_in / 4; the lanes combine by
// butterfly and lane 1 leaves the sums in st_sum / st_max.  The values: lane j computes value j of the row's fourteen (index j >> 1 of
// side j & 1) and, below 6, value j + 8 — two chains per lane instead of seven.  The row: lane j stores o[j], 128 bytes per node at once.
// Same sums (integers), same values (node_feature_at), same rows.  Measured at C3: 12.7 -> 11.9 us, the window not lower in every round —
// so the plan leaves it off (kK3FeatLanesDefault, profiles/k3_forms_ab_c3.txt); SG_K3_FEAT_LANES=1 names it in the development build.
template <int NK>
__device__ __forceinline__ void k3_in_batch(const ulonglong2* p, size_t st, u32 sl0, u32 S_in, u64& dg, u64& c, u64& er, u64& sm, u64& sq, u64& mx) {
    ulonglong2 x[NK][3];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const u32 sl = sl0 + 8 * k;
        const ulonglong2* q = p + (size_t)(sl < S_in ? sl : S_in - 1) * st;
        x[k][0] = q[0]; x[k][1] = q[1]; x[k][2] = q[2];
    }
    // the batch's one wait: no load above may sink below it (the compiler would move a slice's three into the block of its `in` test)
    asm volatile("" : "+v"(x[0][0].x), "+v"(x[0][0].y), "+v"(x[0][1].x), "+v"(x[0][1].y), "+v"(x[0][2].x), "+v"(x[0][2].y) : : "memory");
#pragma unroll
    for (int k = 1; k < NK; k++) asm volatile("" : "+v"(x[k][0].x), "+v"(x[k][0].y), "+v"(x[k][1].x), "+v"(x[k][1].y), "+v"(x[k][2].x), "+v"(x[k][2].y));
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const bool in = sl0 + 8 * k < S_in;
        dg += in ? x[k][0].x : 0; c += in ? x[k][0].y : 0; er += in ? x[k][1].x : 0; sm += in ? x[k][1].y : 0; sq += in ? x[k][2].x : 0;
        mx = in && x[k][2].y > mx ? x[k][2].y : mx;
    }
}
__global__ __launch_bounds__(256) void k3_node_features_lanes(Dev d, u32 nb_nodes, u32 S_in) {
    static_assert(SG_F_IN == 32, "a row is eight float4, one per lane");
    const u32 N = (u32)d.ctr[C_N_NODES], nk = (u32)d.ctr[C_N_KNOWN];
    const u32 j = threadIdx.x & 7u, side = j & 1u;
    for (u32 v0 = blockIdx.x * 32; v0 < N; v0 += nb_nodes * 32) {
        const u32 vl = v0 + (threadIdx.x >> 3);
        const bool live = vl < N;
        const u32 v = live ? vl : N - 1;                             // (a lane past the last node works on the last one and stores nothing: no branch around the loads and shuffles)
        u64* s = d.st_sum + (size_t)v * SG_NODE_STAT_SUM_WORDS;
        // this side's words as they stand (the out side's, and the in side's of the staged pipelines), ahead of the partials: one round trip for both
        const u64 odg = s[ST_OUT_DEG + side], oc = s[ST_OUT_CNT + side], oer = s[ST_OUT_ERR + side], osm = s[ST_OUT_SUM + side], osq = s[ST_OUT_SSQ + side];
        const u64 omx = d.st_max[(size_t)v * 2 + side], al = s[ST_OUT_ALIVE + side];
        u64 dg = 0, c = 0, er = 0, sm = 0, sq = 0, mx = 0;
        if (S_in) {                                                  // deg, cnt, err, sum, ssq, max of the node's in-edges: over the slices (integer: order-free)
            const u32 r = v / K3_IN_NR;
            const ulonglong2* p = reinterpret_cast<const ulonglong2*>(d.in_part + ((size_t)r * S_in * K3_IN_NR + (v - r * K3_IN_NR)) * 6);
            const size_t st = (size_t)K3_IN_NR * 3;                  // (16-byte words per slice)
            u32 base = 0;
            for (; base + 48 < S_in; base += 64) k3_in_batch<8>(p, st, base + j, S_in, dg, c, er, sm, sq, mx);   // 64 slices: 24 loads in flight
            k3_in_batch<6>(p, st, base + j, S_in, dg, c, er, sm, sq, mx);                                         // the last 48 slices or fewer: 18 loads
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) {
                dg += __shfl_xor(dg, m, 64); c += __shfl_xor(c, m, 64); er += __shfl_xor(er, m, 64); sm += __shfl_xor(sm, m, 64); sq += __shfl_xor(sq, m, 64);
                const u64 o = __shfl_xor(mx, m, 64); mx = o > mx ? o : mx;
            }
            if (live && j == 1) { s[ST_IN_DEG] = dg; s[ST_IN_CNT] = c; s[ST_IN_ERR] = er; s[ST_IN_SUM] = sm; s[ST_IN_SSQ] = sq; d.st_max[(size_t)v * 2 + 1] = mx; }
        }
        if (!(S_in && side)) { dg = odg; c = oc; er = oer; sm = osm; sq = osq; mx = omx; }
        const float a0 = node_feature_at(j >> 1, dg, c, er, sm, sq, mx, al);
        const float a1 = j < 6 ? node_feature_at(4 + (j >> 1), dg, c, er, sm, sq, mx, al) : 0.0f;
        // lane j's float4: 0, 1 = first values of lanes 0-3, 4-7; 2, 3, 4 take the second values of lanes (0, 1), (2, 3), (4, 5)
        // (lanes named within the wave: a __shfl of width 8 would be this translation unit's only one, and the other kernels' shuffles compile differently beside it)
        const int l0 = (int)(threadIdx.x & 56u), fa = l0 + (int)(side * 4), b = l0 + (j == 2 ? 0 : j == 3 ? 2 : 4);
        const float f0 = __shfl(a0, fa, 64), f1 = __shfl(a0, fa + 1, 64), f2 = __shfl(a0, fa + 2, 64), f3 = __shfl(a0, fa + 3, 64);
        const float g0 = __shfl(a1, b, 64), g1 = __shfl(a1, b + 1, 64);
        if (!live) continue;
        const u32 kind = v < nk ? d.kind[v] : 0u;
        float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < 2) w = make_float4(f0, f1, f2, f3);
        else if (j == 2) w = make_float4(g0, g1, kind == SG_NODE_POD ? 1.0f : 0.0f, kind == SG_NODE_SERVICE ? 1.0f : 0.0f);
        else if (j == 3) w = make_float4(kind == 0 ? 1.0f : 0.0f, g0, g1, 1.0f);
        else if (j == 4) w = make_float4(g0, g1, 0.0f, 0.0f);
        reinterpret_cast<float4*>(d.x0 + (size_t)v * SG_F_IN)[j] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {                       // the alive list is consumed (k3_in_stats): report and re-arm
        const u64 n = d.ctr[C_ALIVE_N];
        d.ctr[C_ALIVE_SEEN] = n;
        d.ctr[C_ALIVE_DROPPED] = d.ctr[C_ALIVE_DROP] + (n > d.alive_cap ? n - d.alive_cap : 0);
        d.ctr[C_ALIVE_N] = 0; d.ctr[C_ALIVE_DROP] = 0;
    }
}

// window reset in one launch (replaces seven memsets): node arrays, outbound-ip table, window
// counters; for variant 1 also the whole edge table if more edges were found than max_edges.
__global__ __launch_bounds__(256) void k_reset_window(Dev d) {
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, nt = (u64)gridDim.x * 256;
    const u64 nc = (u64)d.ncap + 1;
    // (obkeys must be cleared here, not in K5: k5's rows reference OBIP ranks only, but a K1a of the next
    // window may already be enqueued behind this kernel — same stream, so ordering is by launch order)
    if (!d.dh_g) for (u64 i = tid; i < nc * SG_DEG_REP; i += nt) { d.deg[i * SG_DEG_STRIDE] = 0; if (d.warm) d.deg2[i * SG_DEG_STRIDE] = 0; }    // (dh_g: no degree counters — k2_deg_hist rewrites every count it uses)
    for (u64 i = tid; i < nc; i += nt) d.cursor[i] = 0;
    for (u64 i = tid; i < (u64)d.ncap * SG_NODE_STAT_SUM_WORDS; i += nt) d.st_sum[i] = 0;
    for (u64 i = tid; i < (u64)d.ncap * SG_NODE_STAT_MAX_WORDS; i += nt) d.st_max[i] = 0;
    for (u64 i = tid; i <= d.obmask; i += nt) d.obkeys[i] = 0;
    // a window that is reset WITHOUT having been closed (sg_window_reset on an open window = discard): what the close
    // path would have consumed and re-armed — the per-workgroup K1 statistics, the overflow and alive lists
    for (u64 i = tid; i < (u64)SG_MAX_K1_WGS * WS_WORDS; i += nt) d.wgstat[i] = (i % WS_WORDS) == WS_TMIN ? ~0ull : 0ull;
    if (tid == 0) { d.ctr[C_OVF_N] = 0; d.ctr[C_ALIVE_N] = 0; d.ctr[C_ALIVE_DROP] = 0; }
    if (tid == 0) { d.ctr[C_COLD] = 0; d.ctr[C_DELTA_N] = 0; d.ctr[C_OB_RAW] = 0; }   // what a close without kc_prepare finds in place (sg_k2.h; the reader's copies: C_LAST_*)
    if (d.variant == 1 && d.ctr[C_EDGES_FOUND] > d.max_edges) {
        for (u64 i = tid; i <= d.emask; i += nt) {
            d.ekeys[i] = SG_EKEY_EMPTY;
            ulonglong2* a = reinterpret_cast<ulonglong2*>(d.eacc + (size_t)i * 4);
            a[0] = make_ulonglong2(0, 0); a[1] = make_ulonglong2(0, 0);
            if (d.hist) { uint4* hs = reinterpret_cast<uint4*>(d.hist_src + (size_t)i * SG_HIST_BINS); const uint4 z = make_uint4(0, 0, 0, 0); hs[0] = z; hs[1] = z; hs[2] = z; hs[3] = z; }
        }
    }
}
