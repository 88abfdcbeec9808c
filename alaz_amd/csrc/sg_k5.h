// sg_k5.h — K5 edge_score: per-node projections (MFMA) and the per-edge score
// Part of the kernel translation unit: included by sg_kernels.h (which holds the shared helpers), in this order.
#pragma once

// ------------------------------------------------------------------------------------------------
// K5  edge_score: P = b1 + h Wu, Q = h Wv per node (MFMA), then per edge
//     s = sigmoid(b2 + tree_sum_j( ReLU(P[u][j] + Q[v][j] + sum_k e[k] We[k][j]) * w2[j] )).
// ------------------------------------------------------------------------------------------------
template <bool USE_MFMA>
__global__ __launch_bounds__(256) void k5_node_proj(Dev d, const float* __restrict__ hL, const float* __restrict__ Wh) {
    constexpr int LDA = SG_F_HID + 2;
    __shared__ float A[16 * LDA];
    __shared__ u32 vid[16];
    const bool listed = d.world > 1 && d.ctr[C_ACT_L] != SG_ACT_NONE;   // only the endpoints of this shard's edges
    const u32 N = listed ? (u32)d.ctr[C_ACT_P] : (u32)d.ctr[C_N_NODES];
    const float* __restrict__ Wu = Wh; const float* __restrict__ Wv = Wh + SG_F_HID * SG_F_HID;
    const float* __restrict__ b1 = Wv + SG_F_HID * SG_F_HID + SG_F_EDGE * SG_F_HID;
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (u32 tile = blockIdx.x; tile * 16 < N; tile += gridDim.x) {
        const u32 v0 = tile * 16;
        if (threadIdx.x < 16) vid[threadIdx.x] = v0 + threadIdx.x < N ? (listed ? d.act_p[v0 + threadIdx.x] : v0 + threadIdx.x) : 0u;
        __syncthreads();
        for (u32 idx = threadIdx.x; idx < 16 * SG_F_HID; idx += 256) {
            const u32 r = idx >> 6, k = idx & 63;
            A[r * LDA + k] = (v0 + r < N) ? hL[(size_t)vid[r] * SG_F_HID + k] : 0.0f;
        }
        __syncthreads();
        if (USE_MFMA) {
            const int jb = wave * 16, i = lane & 15;
            const float bj = b1[jb + i];
            f32x4 p = { bj, bj, bj, bj }, q = { 0.0f, 0.0f, 0.0f, 0.0f };
            p = dense_tile_mfma<SG_F_HID>(A, LDA, Wu, jb, p);
            q = dense_tile_mfma<SG_F_HID>(A, LDA, Wv, jb, q);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const u32 row = (lane >> 4) * 4 + r;
                if (v0 + row < N) { d.P[(size_t)vid[row] * SG_F_HID + SG_PQ_POS(jb + i)] = p[r]; d.Q[(size_t)vid[row] * SG_F_HID + SG_PQ_POS(jb + i)] = q[r]; }
            }
        } else {
            const u32 row = threadIdx.x >> 4, jq = (threadIdx.x & 15) * 4;
            float p[4], q[4];
#pragma unroll
            for (int c = 0; c < 4; c++) { p[c] = b1[jq + c]; q[c] = 0.0f; }
            for (int k = 0; k < (int)SG_F_HID; k++) {
                const float a = A[row * LDA + k];
#pragma unroll
                for (int c = 0; c < 4; c++) { p[c] = fmaf(a, Wu[(size_t)k * SG_F_HID + jq + c], p[c]); q[c] = fmaf(a, Wv[(size_t)k * SG_F_HID + jq + c], q[c]); }
            }
            if (v0 + row < N)
#pragma unroll
                for (int c = 0; c < 4; c++) { d.P[(size_t)vid[row] * SG_F_HID + SG_PQ_POS(jq + c)] = p[c]; d.Q[(size_t)vid[row] * SG_F_HID + SG_PQ_POS(jq + c)] = q[c]; }
        }
        __syncthreads();
    }
}

// One wave scores 4 edges per step: 16 lanes per edge, lane q of a group owns hidden units q + 16 m (m = 0..3).
//   t_j = P[u][j] + Q[v][j] + sum_k e_k We[k][j] (fmaf chain over k), ReLU, * w2[j]
//   sum over j in the canonical butterfly order (strides 32, 16, 8, 4, 2, 1): strides 32 and 16 pair units of
//   the SAME lane (j ^ 32 <-> m ^ 2, j ^ 16 <-> m ^ 1), strides 8..1 are DPP steps inside the group's row of 16 lanes — the
//   same additions in the same order as one lane per unit (fp32 addition commutes bitwise), at a quarter of the
//   instructions per edge.  Lane 0 of a group writes the edge's row.
static_assert(sizeof(sg_edge_out) == 64 && offsetof(sg_edge_out, sum_ns) == 0 && offsetof(sg_edge_out, max_ns) == 8 && offsetof(sg_edge_out, sumsq_us) == 16 &&
              offsetof(sg_edge_out, from_ref) == 24 && offsetof(sg_edge_out, to_ref) == 28 && offsetof(sg_edge_out, count) == 32 && offsetof(sg_edge_out, err_count) == 36 &&
              offsetof(sg_edge_out, score) == 40 && offsetof(sg_edge_out, lat_z) == 44 && offsetof(sg_edge_out, err_ratio) == 48 && offsetof(sg_edge_out, alive) == 52 &&
              offsetof(sg_edge_out, p50_us) == 56 && offsetof(sg_edge_out, p99_us) == 60, "k5_edge_score writes a row as eight 8-byte words");
// p50_us | p99_us << 32 of edge ec off its log2 histogram (include/servicegraph.h); 0 for an edge without requests
__device__ __forceinline__ u64 k5_percentiles(const Dev& d, u32 ec, u32 count, u64 max_ns) {
    u64 val = 0;
    if (count) {
        const uint4* hp = reinterpret_cast<const uint4*>(d.hist_csr + (size_t)ec * SG_HIST_BINS);
        const uint4 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3];
        const u32 hb[SG_HIST_BINS] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w, h3.x, h3.y, h3.z, h3.w};
        u64 r50 = ((u64)count * 50 + 99) / 100, r99 = ((u64)count * 99 + 99) / 100;
        r50 = r50 ? r50 : 1; r99 = r99 ? r99 : 1;
        u64 cum = 0; u32 b50 = SG_HIST_BINS - 1, b99 = SG_HIST_BINS - 1; bool f50 = false, f99 = false;
#pragma unroll
        for (u32 b = 0; b < SG_HIST_BINS; b++) { cum += hb[b]; if (!f50 && cum >= r50) { b50 = b; f50 = true; } if (!f99 && cum >= r99) { b99 = b; f99 = true; } }
        u64 e50 = b50 == SG_HIST_BINS - 1 ? max_ns : (1ull << (17 + b50)), e99 = b99 == SG_HIST_BINS - 1 ? max_ns : (1ull << (17 + b99));
        e50 = e50 > max_ns ? max_ns : e50; e99 = e99 > max_ns ? max_ns : e99;
        e50 /= 1000ull; e99 /= 1000ull;
        val = (u64)(e50 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)e50) | ((u64)(e99 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)e99) << 32);
    }
    return val;
}
// Window reset folded into the last kernel of the pipeline (both forms of k5_edge_score): nothing after it reads these arrays;
// the counters stay: sg_window_read / the next kc_prepare consume them — but for the three words at the end.
__device__ __forceinline__ void k5_window_reset(const Dev& d) {
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, nt = (u64)gridDim.x * 256;
    const u64 nc = (u64)d.ncap + 1;
    if (!d.dh_g) for (u64 i = tid; i < nc * SG_DEG_REP; i += nt) { d.deg[i * SG_DEG_STRIDE] = 0; if (d.warm) d.deg2[i * SG_DEG_STRIDE] = 0; }
    for (u64 i = tid; i < nc; i += nt) d.cursor[i] = 0;
    for (u64 i = tid; i < (u64)d.ncap * SG_NODE_STAT_SUM_WORDS; i += nt) d.st_sum[i] = 0;
    for (u64 i = tid; i < (u64)d.ncap * SG_NODE_STAT_MAX_WORDS; i += nt) d.st_max[i] = 0;
    for (u64 i = tid; i <= d.obmask; i += nt) d.obkeys[i] = 0;
    if (tid == 0) { d.ctr[C_COLD] = 0; d.ctr[C_DELTA_N] = 0; d.ctr[C_OB_RAW] = 0; }   // what a close without kc_prepare finds in place (sg_k2.h; the reader's copies: C_LAST_*)
}
template <bool RESET>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k5_edge_score(Dev d, const float* __restrict__ Wh) {
    const u32 E = (u32)d.ctr[C_N_EDGES], nk = (u32)d.ctr[C_N_KNOWN], nl = (u32)d.ctr[C_N_LABELS];
    const float* __restrict__ We = Wh + 2 * SG_F_HID * SG_F_HID;
    const float* __restrict__ w2 = We + SG_F_EDGE * SG_F_HID + SG_F_HID;
    const float b2 = w2[SG_F_HID];
    const u32 lane = threadIdx.x & 63, q = lane & 15, g = lane >> 4;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
    float we[SG_F_EDGE][4], w2r[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        w2r[m] = w2[q + 16 * m];
#pragma unroll
        for (int k = 0; k < (int)SG_F_EDGE; k++) we[k][m] = We[k * SG_F_HID + q + 16 * m];
    }
    // Two steps of four edges per iteration, and the endpoints of the NEXT iteration's edges are fetched while this one's
    // rows are gathered: the dependent chain per iteration is one round trip (the gathers), not two (ids, then gathers).
    // What the 16 lanes of a group need in common is loaded ONCE per group and spread with DPP row_newbcast (a v_mov per value):
    // the two edges' feature vectors are one dword per lane (lanes 0..7 edge A's e_0..e_7, lanes 8..15 edge B's) instead of four
    // 16-byte loads that return the same 32 bytes to all sixteen lanes, the four endpoint ids one dword in lanes 0..3 instead of
    // four loads — 9 memory instructions and 5.5 KiB returned per wave and iteration instead of 15 and 10 KiB (the kernel is
    // bound by the vector-memory pipe, not by HBM: P and Q are L2-resident).
    auto step = [&](const float4 P4, const float4 Q4, const float (&ek)[SG_F_EDGE]) -> float {
        const float pq[4] = {P4.x + Q4.x, P4.y + Q4.y, P4.z + Q4.z, P4.w + Q4.w};
        float r[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            float x = pq[m];
#pragma unroll
            for (int k = 0; k < (int)SG_F_EDGE; k++) x = fmaf(ek[k], we[k][m], x);
            x = x > 0.0f ? x : 0.0f;
            r[m] = x * w2r[m];
        }
        float sum = (r[0] + r[2]) + (r[1] + r[3]);                  // strides 32, then 16
        sum = sum + xor_partner_f32(sum, 8); sum = sum + xor_partner_f32(sum, 4);
        sum = sum + xor_partner_f32(sum, 2); sum = sum + xor_partner_f32(sum, 1);
        return sum;                                                  // (every lane of the 16 holds it)
    };
    static_assert(SG_F_EDGE == 8, "k5_edge_score spreads two 8-float edge feature vectors over a DPP row of 16 lanes");
    const u32* __restrict__ idsrc = (q & 1u) ? d.col : d.csr_from;   // lane q & 3 of a group: from(A), to(A), from(B), to(B)
    // The ROWS of an iteration's eight edges are written by the whole wave: 8 x 64 bytes = 64 lanes x 8 bytes, lane l holds
    // 8-byte word l % 8 of edge l / 8 — one fully coalesced store per iteration instead of four 16-byte stores from one lane in
    // sixteen per step (whose ~100 instructions of row assembly ran with 4 of 64 lanes active).
    //   word 0..2 sum_ns, max_ns, sumsq_us = accumulators 1..3; word 3 from_ref | to_ref; word 4 count | err = accumulator 0;
    //   word 5 score | lat_z; word 6 err_ratio | alive; word 7 p50_us | p99_us
    const u32 wk = lane & 7u, we8 = lane >> 3;
    const u32* __restrict__ srcA = wk == 3 ? d.csr_from : reinterpret_cast<const u32*>(d.errr);
    const u32* __restrict__ srcB = wk == 3 ? d.col : (wk == 5 ? reinterpret_cast<const u32*>(d.latz) : d.alive_csr);
    const u32 accj = wk < 3 ? wk + 1 : 0u;
    const int srcl = (int)(((we8 & 3u) << 4) | (we8 < 4 ? 0u : 8u));     // lane that holds the score sum of this lane's edge: group (edge & 3), its
                                                                         // lower half for the first step's four edges, its upper half for the second's
    if (E) {
        const u32 stride = nw * 8, last = E - 1;
        u32 pa = wave * 8 + g, pb = pa + 4;                          // this iteration's two edges of the lane group (clamped when beyond E)
        // Round 4: TWO iterations in flight.  A wave runs ~30 iterations at C3 and an iteration was one exposed round trip (the gathers:
        // ~2 us) beside ~0.4 us of arithmetic — 73 us of which 60 were latency at four waves per SIMD.  Now the gathers, the feature
        // dword and the row words of iteration i + 1 are issued BEFORE iteration i is computed (a second register set: 21 dwords), its
        // endpoint ids having been fetched an iteration earlier still; loads return in order, so waiting for set i does not wait for
        // set i + 1.  (The set beyond the last iteration is loaded from clamped addresses and dropped.)
        struct K5Set { float4 PA, QA, PB, QB; u32 ew, wa, wb; u64 wacc; };
        auto ids_of = [&](u32 xa, u32 xb) -> u32 { const u32 px = (q & 2u) ? xb : xa; return idsrc[px < E ? px : last]; };
        auto issue = [&](u32 idw_, u32 xa, u32 xb, u32 x0, K5Set& S) {
            u32 ua = dpp32b<0x150>(idw_), va = dpp32b<0x151>(idw_), ub = dpp32b<0x152>(idw_), vb = dpp32b<0x153>(idw_);
            if SG_ABL(d, 0x1000u) { ua &= 15u; va &= 15u; ub &= 15u; vb &= 15u; }   // (diagnostic: gathers that hit the L1)
            const u32 ca = xa < E ? xa : last, cb = xb < E ? xb : last;
            S.PA = reinterpret_cast<const float4*>(d.P + (size_t)ua * SG_F_HID)[q]; S.QA = reinterpret_cast<const float4*>(d.Q + (size_t)va * SG_F_HID)[q];
            S.PB = reinterpret_cast<const float4*>(d.P + (size_t)ub * SG_F_HID)[q]; S.QB = reinterpret_cast<const float4*>(d.Q + (size_t)vb * SG_F_HID)[q];
            S.ew = __float_as_uint(d.efeat[(size_t)(q < 8 ? ca : cb) * SG_F_EDGE + (q & 7u)]);
            // what this lane's row word is made of: fetched beside the gathers
            const u32 er_ = x0 + we8, ec_ = er_ < E ? er_ : last;
            S.wacc = d.acc_csr[(size_t)ec_ * 4 + accj];
            S.wa = srcA[ec_]; S.wb = srcB[ec_];
        };
        // One iteration: `cur` is computed and stored, `nxt` issued; the two sets ALTERNATE between the two calls of the loop body — rotating
        // them through copies at the back edge made the compiler wait for the set in flight there (a v_mov needs its source loaded).
        auto iter = [&](K5Set& cur, K5Set& nxt, const u32 idw_next, u32& idw_after, const u32 p0) {
            const u32 na = pa + stride, nb = pb + stride;
            // the endpoints of the iteration after the next go out FIRST: they are then older than the gathers issued below, and the next
            // iteration's wait for them does not wait for those gathers (issued the other way round, it was a vmcnt(0) at the loop top)
            idw_after = ids_of(na + stride, nb + stride);
            issue(idw_next, na, nb, p0 + stride, nxt);
            __builtin_amdgcn_sched_barrier(0);                       // (the scheduler moved the arithmetic of `cur` above these loads)
            const float4 PA = cur.PA, QA = cur.QA, PB = cur.PB, QB = cur.QB;
            const u32 ew = cur.ew, wa = cur.wa, wb = cur.wb; const u64 wacc = cur.wacc;
            const u32 er = p0 + we8, ec = er < E ? er : last;
            const float eka[SG_F_EDGE] = {__uint_as_float(dpp32b<0x150>(ew)), __uint_as_float(dpp32b<0x151>(ew)), __uint_as_float(dpp32b<0x152>(ew)), __uint_as_float(dpp32b<0x153>(ew)),
                                          __uint_as_float(dpp32b<0x154>(ew)), __uint_as_float(dpp32b<0x155>(ew)), __uint_as_float(dpp32b<0x156>(ew)), __uint_as_float(dpp32b<0x157>(ew))};
            const float ekb[SG_F_EDGE] = {__uint_as_float(dpp32b<0x158>(ew)), __uint_as_float(dpp32b<0x159>(ew)), __uint_as_float(dpp32b<0x15A>(ew)), __uint_as_float(dpp32b<0x15B>(ew)),
                                          __uint_as_float(dpp32b<0x15C>(ew)), __uint_as_float(dpp32b<0x15D>(ew)), __uint_as_float(dpp32b<0x15E>(ew)), __uint_as_float(dpp32b<0x15F>(ew))};
            const float sa = step(PA, QA, eka);
            const float sb = step(PB, QB, ekb);
            const float mysum = __shfl(q < 8 ? sa : sb, srcl, 64);     // ONE shuffle executed by all lanes (two under a select were sunk into exec-masked
                                                                       // branches by the compiler: ds_bpermute returns 0 for an inactive source lane)
            u64 val = wacc;                                          // words 0..2 and 4
            if (wk == 3) val = (u64)ref_of_dense(wa, nk, nl) | ((u64)ref_of_dense(wb, nk, nl) << 32);
            else if (wk == 5) { const float logit = mysum + b2; val = (u64)__float_as_uint(1.0f / (1.0f + expf(-logit))) | ((u64)wb << 32); }
            else if (wk == 6) val = (u64)wa | ((u64)wb << 32);
            else if (wk == 7) {
                val = 0;
                if (d.hist) {                                        // percentiles off the log2 histogram (include/servicegraph.h)
                    const ulonglong2* __restrict__ ac = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)ec * 4);
                    val = k5_percentiles(d, ec, (u32)(ac[0].x & 0xFFFFFFFFull), ac[1].x);
                }
            }
            // The store as a BUFFER store on the wave's 512 bytes of this iteration (p0 is wave-uniform): rows beyond E are dropped by
            // the resource's range check, not by a branch — a branch around the store is a join for the compiler's vmcnt bookkeeping,
            // and the next half-iteration's wait for its endpoint ids then also waited for the first gather of the set in flight.
            {
                const u32 p0u = (u32)__builtin_amdgcn_readfirstlane((int)p0);
                const u32 nrow = SG_ABL(d, 0x2000u) ? 0u : (E - p0u < 8u ? E - p0u : 8u);
                const __amdgpu_buffer_rsrc_t rr_ = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<u64*>(d.rows) + (size_t)p0u * 8, 0, (int)(nrow * 64u), 0x00020000);
                v2u_t dv; dv.x = (u32)val; dv.y = (u32)(val >> 32);
                __builtin_amdgcn_raw_buffer_store_b64(dv, rr_, lane * 8u, 0, 0);
            }
            pa = na; pb = nb;
        };
        K5Set A, B;
        u32 i1 = ids_of(pa + stride, pb + stride), i2;               // the endpoints of iteration 1 ...
        { const u32 id0 = ids_of(pa, pb); issue(id0, pa, pb, wave * 8, A); }   // ... in flight before iteration 0's gathers
        for (u32 p0 = wave * 8; p0 < E; p0 += 2 * stride) {
            iter(A, B, i1, i2, p0);
            if (p0 + stride >= E) break;                             // (uniform)
            iter(B, A, i2, i1, p0 + stride);
        }
    }
    if (RESET) k5_window_reset(d);
}

// ------------------------------------------------------------------------------------------------
// Form 1 of k5_edge_score: ONE LANE PER EDGE, a wave takes 64 consecutive CSR positions per batch.
//   What the sixteen lanes of form 0 share (ids, features, sigmoid, refs, row words) is paid once per 64 edges per wave
//   instruction here, not once per 8.  The weights We[k][j], w2[j] are wave-uniform: scalar loads, SGPR operands of the packed FMAs.
//   P and Q rows are gathered as in form 0 — four lanes on the four 16-byte words of a 64-byte QUARTER row (hidden units
//   q, q+16, q+32, q+48 for q = 4c .. 4c+3), sixteen rows per wave instruction — and dropped into a per-wave LDS tile; each lane
//   reads its own edge's quarter back with ds_read_b128.  The next quarter's gathers are in flight while this one is computed.
//   Tile: 64 quarter rows of P (4 KiB), then 64 of Q; word w of row r lives at 16-byte slot 4 r + (w ^ ((r >> 2) & 3)): the
//   sixteen lanes of a ds_read_b128 group ({0-3, 12-15, 20-27}, ...) then hit sixteen different slots of the 64 banks, and the
//   eight lanes of a ds_write_b128 group still cover 128 contiguous bytes.
//   Sum over j in the canonical order (strides 32, 16, 8, 4, 2, 1): a 16-byte word holds the first two levels of unit q; the
//   quarters are taken in the order 0, 2, 1, 3, so that S_q + S_{q+8} folds as soon as both exist (eight partials live at most).
//   Rounding points as form 0 compiles (default contraction; read from its code): the units q+32 and q+48 enter as rounded
//   products, q and q+16 by a fused multiply-add onto them; the two pair sums and every later level are plain adds.
//   Rows leave as form 0's do: every lane writes its 64-byte row into the (then idle) tile, word w at slot 4 r + (w ^ ((r >> 1) & 3)),
//   the wave reads it back in 8-byte words and issues eight 512-byte buffer stores whose range drops the rows beyond E.
//   EFEAT (Plan::k5_efeat): the lane computes e_uv, lat_z and err_ratio of its own edge itself — edge_feature_values(), sg_k2.h, the
//   arithmetic k3_node_features' edge workgroups run elsewhere — from the accumulators and `from` it loads anyway; no efeat / latz /
//   errr access remains (the arrays do not exist for such an engine).  The feature code keeps its own (default) contraction: the
//   pragma below is lexical.  Same rows, byte for byte (tests/test_gpu_k5_efeat.py).
// ------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef u32 v4u_t __attribute__((ext_vector_type(4)));
#define K5L_WAVE_LDS 8192u                    // bytes of LDS per wave (sg_plan.hpp kK5LanesWgLds = 4 waves of it)
// orders the wave's LDS traffic for the compiler (the hardware runs a wave's DS instructions in order)
__device__ __forceinline__ void k5l_lds_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

template <bool RESET, bool EFEAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k5_edge_score_lanes(Dev d, const float* __restrict__ Wh) {
#pragma clang fp contract(off)
    static_assert(SG_F_HID == 64 && SG_F_EDGE == 8, "k5_edge_score_lanes: 64 hidden units in four quarters, eight edge features");
    __shared__ __attribute__((aligned(256))) f32x4 lds[4 * K5L_WAVE_LDS / 16];
    const u32 E = (u32)d.ctr[C_N_EDGES], nk = (u32)d.ctr[C_N_KNOWN], nl = (u32)d.ctr[C_N_LABELS];
    const float* __restrict__ We = Wh + 2 * SG_F_HID * SG_F_HID;
    const float* __restrict__ w2 = We + SG_F_EDGE * SG_F_HID + SG_F_HID;
    const float b2 = w2[SG_F_HID];
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
    f32x4* const tile = lds + (threadIdx.x >> 6) * (K5L_WAVE_LDS / 16);
    if (E) {
        const u32 last = E - 1, nbatch = (E + 63u) >> 6;
        const u32 sub = lane >> 2, pc = lane & 3u;                  // gathers: instruction i takes row 16 i + sub, its word pc
        const u32 wslot = sub * 4 + (pc ^ ((sub >> 2) & 3u));        // ... and drops it at slot 64 i + wslot (P; Q: + 256)
        const u32 rx = (lane >> 2) & 3u;                            // reads: this lane's row is `lane`
        const u32 ox = (lane >> 1) & 3u;                            // row tile (out): swizzle of this lane's row
        const u32 rb = (((lane >> 3) * 4 + (((lane & 7u) >> 1) ^ ((lane >> 4) & 3u))) << 1) | (lane & 1u);   // read-back: 8-byte word lane & 7 of row 8 j + lane / 8
        // EFEAT: these lane-derived values are worked out again where they are used, from a lane number the optimiser cannot see through
        // (relane), so that they are not kept in registers across the batch loop — a dozen registers that the fp64 chains of the features need
        // to fit the 168 of three waves per SIMD without scratch.  The other instantiations keep the values above (and their code).
        auto relane = [&]() -> u32 { u32 l = lane; asm volatile("" : "+v"(l)); return l; };
        u32 gu[4], gv[4];
        f32x4 R[8];
        auto load_ids = [&](u32 p0) {
            u32 subl = 0;
            if constexpr (EFEAT) subl = relane() >> 2;
#pragma unroll
            for (int i = 0; i < 4; i++) { const u32 p = EFEAT ? p0 + i * 16 + subl : p0 + i * 16 + sub, c = p < E ? p : last; gu[i] = d.csr_from[c]; gv[i] = d.col[c]; }
        };
        // (32-bit byte offsets from P and Q: one register per gather address, the base in scalar registers — the plan takes this form only
        // where a row's offset fits 32 bits, sg_plan.hpp)
        auto row_offsets = [&]() {
            u32 pc_ = pc;
            if constexpr (EFEAT) pc_ = relane() & 3u;
#pragma unroll
            for (int i = 0; i < 4; i++) { gu[i] = gu[i] * (SG_F_HID * 4u) + pc_ * 16u; gv[i] = gv[i] * (SG_F_HID * 4u) + pc_ * 16u; }
        };
        auto issue = [&](int c) {                                   // the gathers of quarter c for the ids at hand
#pragma unroll
            for (int i = 0; i < 4; i++) {
                R[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(d.P) + gu[i] + c * 64);
                R[4 + i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(d.Q) + gv[i] + c * 64);
            }
        };
        float S[8];                                                 // partial sums: [0..3] units 4c.. of quarters 0 / 2, [4..7] of quarters 1 / 3
        float ek[SG_F_EDGE];
        // one quarter: S_q (levels 32 and 16 of the sum) for q = 4 c + w, w = 0..3, into out[0..3]
        // The weights stream through scalar registers in blocks of sixteen — We[4 kh .. 4 kh + 3][4 c + 16 m .. + 3], four s_load_dwordx4 —,
        // block i + 1 requested once block i has arrived and before it is used (scalar loads return out of order: a wait for them is
        // lgkmcnt(0), so nothing may be in flight behind the block that is waited for).  Left to itself the compiler hoists the loads —
        // out of the batch loop, or a quarter's 144 values at once — and spills them to lanes of vector registers, a v_readlane pair per
        // packed FMA: the offset goes through an asm the optimiser cannot see through, and scheduling barriers fence every block.
        auto quarter = [&](int c, float (&out)[4]) {
            f32x4 pq[4];                                             // P[u] + Q[v], units 4c + w + 16 m at [w][m]
            u32 rd = lane * 4 + rx;
            if (EFEAT) { const u32 l = relane(); rd = l * 4 + ((l >> 2) & 3u); }
#pragma unroll
            for (int w = 0; w < 4; w++) pq[w] = tile[rd ^ (u32)w] + tile[256 + (rd ^ (u32)w)];
            f32x4 W[2][4], w2v[4];
            auto wload = [&](int blk, f32x4 (&dst)[4]) {
                u32 o = (u32)((blk & 1) * 4 * SG_F_HID + 16 * (blk >> 1) + 4 * c);
                asm volatile("" : "+s"(o));                          // (one per block: instruction selection orders loads of constant memory by nothing else)
#pragma unroll
                for (int i = 0; i < 4; i++) dst[i] = *reinterpret_cast<const f32x4*>(We + o + i * SG_F_HID);
            };
            wload(0, W[0]);
            f32x2 xa[4], xb[4], ta, tb;                              // units (4c, 4c+1) and (4c+2, 4c+3), each + 16 m
#pragma unroll
            for (int blk = 0; blk < 8; blk++) {
                const int m = blk >> 1, kh = blk & 1;
                __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): this block's weights (and, at first, the tile reads)
                if (blk < 7) wload(blk + 1, W[(blk + 1) & 1]);
                else {
                    u32 o = (u32)(4 * c);
                    asm volatile("" : "+s"(o));
#pragma unroll
                    for (int i = 0; i < 4; i++) w2v[i] = *reinterpret_cast<const f32x4*>(w2 + o + 16 * i);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (kh == 0) { ta = (f32x2){ pq[0][m], pq[1][m] }; tb = (f32x2){ pq[2][m], pq[3][m] }; }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const f32x2 ee = { ek[kh * 4 + i], ek[kh * 4 + i] };
                    ta = __builtin_elementwise_fma(ee, W[blk & 1][i].xy, ta);
                    tb = __builtin_elementwise_fma(ee, W[blk & 1][i].zw, tb);
                }
                if (kh == 1) { ta = __builtin_elementwise_max(ta, (f32x2){ 0.0f, 0.0f }); tb = __builtin_elementwise_max(tb, (f32x2){ 0.0f, 0.0f }); }
                asm volatile("" : "+v"(ta), "+v"(tb));                 // (... and the arithmetic by this: the block's FMAs stay inside its fences)
                if (kh == 1) { xa[m] = ta; xb[m] = tb; }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            // stride 32: unit q + 32 a rounded product, unit q fused onto it (q + 48 and q + 16 likewise); stride 16: a plain add
            const f32x2 sa = __builtin_elementwise_fma(w2v[0].xy, xa[0], w2v[2].xy * xa[2]) + __builtin_elementwise_fma(w2v[1].xy, xa[1], w2v[3].xy * xa[3]);
            const f32x2 sb = __builtin_elementwise_fma(w2v[0].zw, xb[0], w2v[2].zw * xb[2]) + __builtin_elementwise_fma(w2v[1].zw, xb[1], w2v[3].zw * xb[3]);
            out[0] = sa.x; out[1] = sa.y; out[2] = sb.x; out[3] = sb.y;
        };
        u32 b = wave;
        // EFEAT: what edge_feature_values() takes for this lane's edge of the batch at hand — its accumulators and its row's mean / deviation —,
        // fetched a batch ahead: `from` beside the next batch's ids (quarter 1), the rest behind it, late in the row's assembly.  The
        // dependent round trips (from, then row_mu / row_sd) are over before the batch that needs them has staged its quarter 0.
        u32 nfrom = 0; ulonglong2 nx = {0, 0}, ny = {0, 0}; double nmu = 0.0, nsd = 0.0;
        auto load_own = [&](u32 c) {
            nx = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)c * 4)[0]; ny = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)c * 4)[1];
            nmu = d.row_mu[nfrom]; nsd = d.row_sd[nfrom];
        };
        if (b < nbatch) {
            if (EFEAT) { const u32 c0 = b * 64u + lane < E ? b * 64u + lane : last; nfrom = d.csr_from[c0]; load_own(c0); }
            load_ids(b * 64u); row_offsets(); issue(0);
        }
        for (; b < nbatch; b += nw) {
            const u32 p0 = b * 64u;
            const u32 er = p0 + lane, ec = er < E ? er : last;
            const u32 np0 = b + nw < nbatch ? (b + nw) * 64u : last;            // the next batch of this wave (beyond the last: clamped, dropped)
            // this lane's own edge: 32 bytes of features, 32 of accumulators, five dwords — all coalesced across the wave
            const u32 nec = EFEAT ? (np0 + lane < E ? np0 + lane : last) : 0u;                 // (EFEAT: this lane's edge of the next batch)
            f32x4 e0, e1; u32 wer, wlz;
            if (!EFEAT) { e0 = reinterpret_cast<const f32x4*>(d.efeat + (size_t)ec * SG_F_EDGE)[0]; e1 = reinterpret_cast<const f32x4*>(d.efeat + (size_t)ec * SG_F_EDGE)[1]; }
            float T[4];
            // quarters 0, 2, 1, 3: stage the quarter whose gathers are in the registers, send the next one's, compute
#define K5L_STAGE(C, NEXT) { k5l_lds_order();                                                                                \
                u32 ws_ = wslot; if (EFEAT) { const u32 l = relane(), s_ = l >> 2; ws_ = s_ * 4 + ((l & 3u) ^ ((s_ >> 2) & 3u)); }           \
                _Pragma("unroll") for (int i = 0; i < 4; i++) { tile[64 * i + ws_] = R[i]; tile[256 + 64 * i + ws_] = R[4 + i]; } \
                k5l_lds_order(); NEXT; __builtin_amdgcn_sched_barrier(0); }
            // EFEAT: the features of the lane's own edge go between quarter 0's staging and quarter 2's gathers — the one place of the batch
            // where the eight gather registers R are dead, which is what the fp64 chains need to fit the 168 registers of three waves per SIMD
            auto features = [&]() {
                EdgeFeat f;
                edge_feature_values(d, nx, ny, [&](double& mu_, double& sd_) { mu_ = nmu; sd_ = nsd; }, f);
                e0 = (f32x4){ f.w0.x, f.w0.y, f.w0.z, f.w0.w }; e1 = (f32x4){ f.w1.x, f.w1.y, f.w1.z, f.w1.w };
                wlz = __float_as_uint(f.lat_z); wer = __float_as_uint(f.err_ratio);
                __builtin_amdgcn_sched_barrier(0);
            };
            K5L_STAGE(0, { if (EFEAT) features(); issue(2); })
            ek[0] = e0[0]; ek[1] = e0[1]; ek[2] = e0[2]; ek[3] = e0[3]; ek[4] = e1[0]; ek[5] = e1[1]; ek[6] = e1[2]; ek[7] = e1[3];
            { float o[4]; quarter(0, o); S[0] = o[0]; S[1] = o[1]; S[2] = o[2]; S[3] = o[3]; }
            K5L_STAGE(2, issue(1))
            { float o[4]; quarter(2, o); for (int i = 0; i < 4; i++) S[i] = S[i] + o[i]; }                  // stride 8: units 0..3 with 8..11
            K5L_STAGE(1, { issue(3); load_ids(np0); if (EFEAT) nfrom = d.csr_from[nec]; })
            { float o[4]; quarter(1, o); S[4] = o[0]; S[5] = o[1]; S[6] = o[2]; S[7] = o[3]; }
            // ... the accumulators and five dwords of it: wanted at the end only, fetched beside the last quarter's arithmetic
            const ulonglong2 a01 = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)ec * 4)[0], a23 = reinterpret_cast<const ulonglong2*>(d.acc_csr + (size_t)ec * 4)[1];
            const u32 mu = d.csr_from[ec], mv = d.col[ec];
            if (!EFEAT) { wer = reinterpret_cast<const u32*>(d.errr)[ec]; wlz = reinterpret_cast<const u32*>(d.latz)[ec]; }
            const u32 wal = d.alive_csr[ec];
            K5L_STAGE(3, { row_offsets(); issue(0); })                                                                      // (the next batch's first quarter)
            { float o[4]; quarter(3, o); for (int i = 0; i < 4; i++) S[4 + i] = S[4 + i] + o[i]; }          // stride 8: units 4..7 with 12..15
#undef K5L_STAGE
#pragma unroll
            for (int i = 0; i < 4; i++) T[i] = S[i] + S[4 + i];                                             // stride 4
            const float sum = (T[0] + T[2]) + (T[1] + T[3]);                                               // strides 2, 1
            const float logit = sum + b2;
            const u32 score = __float_as_uint(1.0f / (1.0f + expf(-logit)));
            const u64 refs = (u64)ref_of_dense(mu, nk, nl) | ((u64)ref_of_dense(mv, nk, nl) << 32);
            u64 pct = 0;
            if (d.hist) pct = k5_percentiles(d, ec, (u32)(a01.x & 0xFFFFFFFFull), a23.x);
            // the row: words 0..2 sum_ns, max_ns, sumsq_us = accumulators 1..3; 3 from_ref | to_ref; 4 count | err = accumulator 0;
            // 5 score | lat_z; 6 err_ratio | alive; 7 p50_us | p99_us
            // (the next batch's accumulators and row statistics go out HERE: behind the percentiles, the registers' high-water mark of the
            // row's assembly, and with the row's staging and eight stores still between them and their use)
            if (EFEAT) load_own(nec);
            v4u_t* const ot = reinterpret_cast<v4u_t*>(tile);
            u32 ln = lane, ox_ = ox, rb_ = rb;
            if (EFEAT) { ln = relane(); ox_ = (ln >> 1) & 3u; rb_ = (((ln >> 3) * 4 + (((ln & 7u) >> 1) ^ ((ln >> 4) & 3u))) << 1) | (ln & 1u); }
            k5l_lds_order();
            ot[(ln * 4 + ox_) ^ 0u] = (v4u_t){ (u32)a01.y, (u32)(a01.y >> 32), (u32)a23.x, (u32)(a23.x >> 32) };
            ot[(ln * 4 + ox_) ^ 1u] = (v4u_t){ (u32)a23.y, (u32)(a23.y >> 32), (u32)refs, (u32)(refs >> 32) };
            ot[(ln * 4 + ox_) ^ 2u] = (v4u_t){ (u32)a01.x, (u32)(a01.x >> 32), score, wlz };
            ot[(ln * 4 + ox_) ^ 3u] = (v4u_t){ wer, wal, (u32)pct, (u32)(pct >> 32) };
            k5l_lds_order();
            {
                const u32 p0u = (u32)__builtin_amdgcn_readfirstlane((int)p0);
                const u32 nrow = SG_ABL(d, 0x2000u) ? 0u : (E - p0u < 64u ? E - p0u : 64u);
                const __amdgpu_buffer_rsrc_t rr_ = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<u64*>(d.rows) + (size_t)p0u * 8, 0, (int)(nrow * 64u), 0x00020000);
                const v2u_t* const rt = reinterpret_cast<const v2u_t*>(tile);
#pragma unroll
                for (int j = 0; j < 8; j++) __builtin_amdgcn_raw_buffer_store_b64(rt[64 * j + rb_], rr_, (u32)j * 512u + ln * 8u, 0, 0);
            }
        }
    }
    if (RESET) k5_window_reset(d);
}
