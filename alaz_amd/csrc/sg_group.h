// sg_group.h — K14: the window's rows contracted to workloads on the device (include/servicegraph.h, "groups").
// Part of the kernel translation unit: included after sg_track.h.
//
// A row's key is gk(from) << kb | gk(to), kb = bits(GK - 1): u32 while 2 kb <= 32, else u64 (the plan picks the instantiation).
// The rows are sorted by it with a stable LSD radix sort, 8 bits a pass, carrying the row index: the sorted indices are perm.  A
// pass is three plain launches over tiles of K14_TILE positions; E is read from the window's counters and workgroups beyond it
// exit, so a small window costs launches only:
//
//   k14_keys     key and index of every row, into ping-pong buffer 0
//   k14_hist     the tile's digit counts -> hist[digit][tile] (tiles = the window's, not the capacity's); positions beyond E count
//                in no digit
//   k14_scan     (1 workgroup) exclusive scan of hist in place, digit-major: where each (digit, tile) begins in the output
//   k14_scatter  position p of a tile belongs to wave p / (64 K14_ITEMS), round (p / 64) % K14_ITEMS, lane p % 64 — ascending
//                position is ascending (wave, round, lane).  Per wave a digit table in LDS: first the digit counts (LDS atomics),
//                turned into each wave's first output position per digit (the tile's start from hist, plus the waves before it); then
//                round by round the lanes with the same digit find each other with eight 64-bit ballots, rank themselves by lane
//                and the lowest of them moves the wave's table on.  So equal digits keep their order: the pass is stable.  The last
//                pass writes its indices to the slot's perm; its keys are in buffer passes & 1
//   k14_heads    a head is a position whose key differs from the one before it (position 0 is one).  Heads per chunk of K14_CHUNK
//                positions and per workgroup (cpw chunks each, at most 1024 workgroups), for k9_scan (sg_nodes.h, unchanged)
//   k14_fold     k9_out's fold over the sorted positions, the rows gathered through perm: a run inside a thread's span is stored
//                by that thread, a run cut by span boundaries is folded in LDS with integer atomics.  The (at most two) runs cut by
//                the chunk's ends go to the chunk's two partials with plain stores — no device atomic at all, and nothing to zero
//                between windows.  Also row_group[perm[p]] and first
//   k14_stitch   one thread per chunk in which a cut run begins: it adds the partials of the chunks the run goes on through and
//                stores the group edge
#pragma once

#define K14_THREADS 256
#define K14_ITEMS 16                               // positions per thread of a sort tile
#define K14_TILE (K14_THREADS * K14_ITEMS)
#define K14_WAVES (K14_THREADS / 64)
#define K14_ROWS 8                                 // positions per thread of k14_fold
#define K14_CHUNK (K14_THREADS * K14_ROWS)
#define K14_SCAN_THREADS 1024
#define K14_KEY_ROWS 4                             // rows per thread of k14_keys

// a run's accumulator: sg_group_edge with the worst-row key in place of (worst_row, score_max); an LDS slot, a partial
struct K14Acc { u64 cnt, err, sum, ssq, max, q32; u32 from, to, edges, fnodes, first, alive; u64 worst; };
static_assert(sizeof(K14Acc) == 80 && sizeof(sg_group_edge) == 80 && offsetof(sg_group_edge, from_ref) == 48 && offsetof(sg_group_edge, worst_row) == 72,
              "sg_group_edge layout");
#define K14_TAIL_OUT 1u                            // meta flags: the chunk's last run goes on in the next chunk ...
#define K14_THROUGH  2u                            // ... and it began before the chunk: the chunk is inside one run

struct GroupArgs {
    NodesArgs nd;                 // rows, ctr, max_edges, the id ranges; blk and count for k9_scan (the group edge count)
    const u32* map;               // [max_known] group per KNOWN id, SG_NO_GROUP: none
    u32 max_groups, gk, kb;       // GK = max_groups + ncap; kb = bits(GK - 1)
    u32 cpw;                      // chunks per workgroup of k14_heads
    u32 max_chunks;
    u32* hist;                    // [256][tiles]
    u32* chunkcnt;                // [chunks] heads per chunk
    K14Acc* part;                 // [chunks][2]: the run that began before the chunk; the run that goes on behind it
    uint2* meta;                  // [chunks] {group edge of the run that goes on, flags}
    sg_group_edge* out;           // this window's group edges
    u32* row_group;               // [max_edges]
    u32* perm;                    // [max_edges]
};

__device__ __forceinline__ u64 k14_rows_of(const GroupArgs& a) { return k9_rows_of(a.nd); }
__device__ __forceinline__ u32 k14_gk(const GroupArgs& a, u32 ref) {
    const u32 k = k9_node(a.nd, ref);
    if (k == SG_NONE) return a.gk - 1;                               // (a ref beyond the id spaces: no window has one)
    if (SG_REF_TYPE(ref) == SG_REF_KNOWN) { const u32 g = a.map[k]; if (g != SG_NO_GROUP) return g; }
    return a.max_groups + k;
}
__device__ __forceinline__ u32 k14_gref(const GroupArgs& a, u32 ref) {
    if (SG_REF_TYPE(ref) != SG_REF_KNOWN || SG_REF_VALUE(ref) >= a.nd.mk) return ref;
    const u32 g = a.map[SG_REF_VALUE(ref)];
    return g != SG_NO_GROUP ? SG_MAKE_REF(SG_REF_GROUP, g) : ref;
}

template <class KT>
__global__ __launch_bounds__(K14_THREADS) void k14_keys(GroupArgs a, KT* keys, u32* idx) {
    const u64 E = k14_rows_of(a);
    const u64 b = (u64)blockIdx.x * (K14_THREADS * K14_KEY_ROWS);
    if (b >= E) return;
#pragma unroll
    for (int q = 0; q < K14_KEY_ROWS; q++) {
        const u64 j = b + (u64)q * K14_THREADS + threadIdx.x;
        if (j < E) {
            const u64 ft = reinterpret_cast<const u64*>(a.nd.rows + j)[3];   // from_ref | to_ref << 32
            keys[j] = ((KT)k14_gk(a, (u32)ft) << a.kb) | (KT)k14_gk(a, (u32)(ft >> 32));
            idx[j] = (u32)j;
        }
    }
}

template <class KT>
__global__ __launch_bounds__(K14_THREADS) void k14_hist(GroupArgs a, const KT* keys, u32 shift) {
    __shared__ u32 h[256];
    const u64 E = k14_rows_of(a);
    const u64 b = (u64)blockIdx.x * K14_TILE;
    if (b >= E) return;
    const u32 t = threadIdx.x, T = (u32)((E + K14_TILE - 1) / K14_TILE);
    h[t] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K14_ITEMS; i++) {
        const u64 p = b + (u64)i * K14_THREADS + t;
        if (p < E) atomicAdd(&h[(u32)(keys[p] >> shift) & 255u], 1u);
    }
    __syncthreads();
    a.hist[(size_t)t * T + blockIdx.x] = h[t];
}

__global__ __launch_bounds__(K14_SCAN_THREADS) void k14_scan(GroupArgs a) {
    __shared__ u32 wsum[K14_SCAN_THREADS / 64 + 1];
    const u64 E = k14_rows_of(a);
    const u32 t = threadIdx.x, T = (u32)((E + K14_TILE - 1) / K14_TILE);
    const u32 n = 256u * T, per = (n + K14_SCAN_THREADS - 1) / K14_SCAN_THREADS;   // (T <= max_edges / 4096: n fits)
    const u32 i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    u32 s = 0;
    for (u32 i = i0; i < i1; i++) s += a.hist[i];
    u32 tot;
    u32 x = block_excl_scan<K14_SCAN_THREADS>(s, wsum, &tot);
    for (u32 i = i0; i < i1; i++) { const u32 c = a.hist[i]; a.hist[i] = x; x += c; }
}

template <class KT>
__global__ __launch_bounds__(K14_THREADS) void k14_scatter(GroupArgs a, const KT* keys, const u32* idx, KT* keys_out, u32* idx_out, u32 shift) {
    __shared__ u32 wh[K14_WAVES][256];
    const u64 E = k14_rows_of(a);
    const u64 b = (u64)blockIdx.x * K14_TILE;
    if (b >= E) return;
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6, T = (u32)((E + K14_TILE - 1) / K14_TILE);
    for (int w = 0; w < K14_WAVES; w++) wh[w][t] = 0;
    __syncthreads();
    const u64 p0 = b + (u64)wave * (64 * K14_ITEMS) + lane;          // position of round i: p0 + 64 i
    KT k[K14_ITEMS];
#pragma unroll
    for (int i = 0; i < K14_ITEMS; i++) {
        const u64 p = p0 + 64u * i;
        k[i] = p < E ? keys[p] : (KT)0;
        if (p < E) atomicAdd(&wh[wave][(u32)(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {
        u32 off = a.hist[(size_t)t * T + blockIdx.x];                // digit t: where this tile's begin, then each wave's
        for (int w = 0; w < K14_WAVES; w++) { const u32 c = wh[w][t]; wh[w][t] = off; off += c; }
    }
    __syncthreads();
    volatile u32* my = wh[wave];
#pragma unroll
    for (int i = 0; i < K14_ITEMS; i++) {
        const u64 p = p0 + 64u * i;
        const bool v = p < E;
        const u32 d = (u32)(k[i] >> shift) & 255u;
        u64 m = __ballot(v);                                         // the valid lanes with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const u64 bal = __ballot(v && one);
            m &= one ? bal : ~bal;
        }
        const u32 below = (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u32 pre = v ? my[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (v && below == 0) my[d] = pre + (u32)__popcll(m);         // (one lane per digit; the wave's LDS accesses stay in order)
        __builtin_amdgcn_wave_barrier();
        const u32 pos = pre + below;
        if (v && pos < E) { keys_out[pos] = k[i]; idx_out[pos] = idx[p]; }
    }
}

template <class KT>
__global__ __launch_bounds__(K14_THREADS) void k14_heads(GroupArgs a, const KT* keys) {
    __shared__ u32 ws[K14_WAVES];
    const u64 E = k14_rows_of(a);
    const u32 t = threadIdx.x;
    u32 total = 0;                                                   // (thread 0's)
    for (u32 q = 0; q < a.cpw; q++) {
        const u32 c = blockIdx.x * a.cpw + q;
        const u64 c0 = (u64)c * K14_CHUNK;
        if (c >= a.max_chunks || c0 >= E) break;                     // (uniform)
        u32 n = 0;
#pragma unroll
        for (int i = 0; i < K14_ROWS; i++) {
            const u64 p = c0 + (u64)i * K14_THREADS + t;
            if (p < E) n += (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
        }
        n = wave_sum_u32(n);
        if ((t & 63) == 0) ws[t >> 6] = n;
        __syncthreads();
        if (t == 0) {
            u32 s = 0;
            for (int w = 0; w < K14_WAVES; w++) s += ws[w];
            a.chunkcnt[c] = s;
            total += s;
        }
        __syncthreads();
    }
    if (t == 0) a.nd.blk[blockIdx.x] = total;                        // (every workgroup: k9_scan reads them all)
}

__device__ __forceinline__ void k14_zero(K14Acc& s) { s.cnt = s.err = s.sum = s.ssq = s.max = s.q32 = s.worst = 0; s.from = s.to = s.edges = s.fnodes = s.first = s.alive = 0; }
__device__ __forceinline__ void k14_add(K14Acc& s, const K9Row& r, u32 row, bool fnode) {
    s.edges += 1u; s.fnodes += fnode ? 1u : 0u; s.alive += r.alive; s.cnt += r.cnt; s.err += r.err; s.sum += r.sum; s.ssq += r.ssq;
    s.max = r.max > s.max ? r.max : s.max;
    s.q32 += k9_q32(r.score);
    const u64 k = k9_worst_key(r.score, row);
    s.worst = k > s.worst ? k : s.worst;
}
// the sums and maxima of o into s (from, to and first stay: they belong to the part that holds the run's head)
__device__ __forceinline__ void k14_merge(K14Acc& s, const K14Acc& o) {
    s.edges += o.edges; s.fnodes += o.fnodes; s.alive += o.alive; s.cnt += o.cnt; s.err += o.err; s.sum += o.sum; s.ssq += o.ssq; s.q32 += o.q32;
    s.max = o.max > s.max ? o.max : s.max;
    s.worst = o.worst > s.worst ? o.worst : s.worst;
}
// p points to LDS: order-free integer adds and maxima
__device__ __forceinline__ void k14_lds_merge(K14Acc* p, const K14Acc& o) {
    atomicAdd(&p->edges, o.edges);
    if (o.fnodes) atomicAdd(&p->fnodes, o.fnodes);
    if (o.alive) atomicAdd(&p->alive, o.alive);
    atomicAdd(&p->cnt, o.cnt);
    if (o.err) atomicAdd(&p->err, o.err);
    atomicAdd(&p->sum, o.sum); atomicAdd(&p->ssq, o.ssq); atomicAdd(&p->q32, o.q32);
    atomicMax(&p->max, o.max); atomicMax(&p->worst, o.worst);
}
// group edge g of the window (g < E <= max_edges by construction; the test keeps a stray index inside the buffer)
__device__ __forceinline__ void k14_store(const GroupArgs& a, u32 g, const K14Acc& s) {
    if (g >= a.nd.max_edges) return;
    sg_group_edge* p = a.out + g;
    sg_group_edge o;
    o.count = s.cnt; o.err_count = s.err; o.sum_ns = s.sum; o.sumsq_us = s.ssq; o.max_ns = s.max; o.score_q32 = s.q32;
    o.from_ref = s.from; o.to_ref = s.to; o.edges = s.edges; o.from_nodes = s.fnodes; o.first = s.first; o.alive = s.alive;
    o.worst_row = ~(u32)s.worst; o.score_max = k9_key_score((u32)(s.worst >> 32));
    *p = o;
}

template <class KT>
__global__ __launch_bounds__(K14_THREADS) void k14_fold(GroupArgs a, const KT* keys) {
    // slot b: the run whose first crossed span boundary is b (0 = the chunk's start: a run that began in an earlier chunk)
    __shared__ K14Acc slot[K14_THREADS + 1];
    __shared__ u32 sgrp[K14_THREADS + 1];
    __shared__ u32 wmax[K14_WAVES];
    __shared__ u32 wsum[K14_WAVES + 1];
    __shared__ u32 tail_slot, tail_out;
    const u64 E = k14_rows_of(a);
    const u32 c = blockIdx.x;
    const u64 c0 = (u64)c * K14_CHUNK;
    if (c0 >= E) return;                                             // (uniform)
    const u64 c1 = c0 + K14_CHUNK < E ? c0 + K14_CHUNK : E;
    const u32 t = threadIdx.x;
    for (u32 s = t; s <= K14_THREADS; s += K14_THREADS) { k14_zero(slot[s]); sgrp[s] = SG_NONE; }
    u32 base = a.nd.blk[K9_MAX_WGS + c / a.cpw];                     // heads in front of the chunk
    for (u32 q = c / a.cpw * a.cpw; q < c; q++) base += a.chunkcnt[q];
    const u64 j0 = c0 + (u64)t * K14_ROWS;
    const u32 n = j0 < c1 ? (u32)((c1 - j0) < K14_ROWS ? (c1 - j0) : K14_ROWS) : 0u;
    const u64 j1 = j0 + n;
    K9Row r[K14_ROWS];
    KT kk[K14_ROWS];
    u32 pm[K14_ROWS];
#pragma unroll
    for (int q = 0; q < K14_ROWS; q++) {
        if ((u32)q < n) { kk[q] = keys[j0 + q]; pm[q] = a.perm[j0 + q]; r[q] = k9_load(a.nd, pm[q]); }
        else { kk[q] = (KT)0; pm[q] = 0; }
    }
    const bool has_prev = n && j0 > 0;
    const KT kprev = has_prev ? keys[j0 - 1] : (KT)0;
    const u32 fprev = has_prev ? (u32)reinterpret_cast<const u64*>(a.nd.rows + a.perm[j0 - 1])[3] : 0u;   // from_ref of the position before
    const bool flows = n && j1 < E && keys[j1] == kk[n - 1];         // the last run goes on past this span
    const bool first_head = n && (j0 == 0 || kprev != kk[0]);        // a run begins at j0
    u32 heads = first_head ? 1u : 0u;
#pragma unroll
    for (int q = 1; q < K14_ROWS; q++) heads += ((u32)q < n && kk[q] != kk[q - 1]) ? 1u : 0u;
    u32 tot;
    u32 g = base + block_excl_scan<K14_THREADS>(heads, wsum, &tot) - 1u;   // the group edge of the position before j0
    const u32 before = k9_block_excl_max<K14_THREADS>(heads ? t + 1 : 0u, wmax);   // (its __syncthreads also orders the slot init)
    const u32 slot_first = first_head ? t + 1 : before;             // the slot of the run that holds j0, if it is cut
    if (n) {
        K14Acc acc; k14_zero(acc);
        bool here = first_head;                                      // the current run began inside this span
        auto fold = [&](bool cut, u32 s) {
            if (!cut) { k14_store(a, g, acc); return; }        // the whole run is in this span: its only writer
            k14_lds_merge(&slot[s], acc);
            sgrp[s] = g;
            if (here) { slot[s].from = acc.from; slot[s].to = acc.to; slot[s].first = acc.first; }   // (the run's head is here only)
        };
#pragma unroll
        for (int q = 0; q < K14_ROWS; q++) {
            if ((u32)q >= n) break;
            const bool head = q == 0 ? first_head : kk[q] != kk[q - 1];
            if (head) {
                if (q > 0) { fold(!here, slot_first); k14_zero(acc); here = true; }
                g += 1u;
                acc.from = k14_gref(a, r[q].from); acc.to = k14_gref(a, r[q].to); acc.first = (u32)(j0 + q);
            }
            const u32 fb = q == 0 ? fprev : r[q > 0 ? q - 1 : 0].from;
            k14_add(acc, r[q], pm[q], head || r[q].from != fb);
            a.row_group[pm[q]] = g;
        }
        fold(flows || !here, here ? t + 1 : slot_first);
        if (j1 == c1) { tail_slot = here ? t + 1 : slot_first; tail_out = flows ? 1u : 0u; }
    }
    __syncthreads();
    for (u32 s = t; s <= K14_THREADS; s += K14_THREADS) {
        const u32 v = sgrp[s];
        if (v == SG_NONE) continue;
        if (s == 0) a.part[(size_t)c * 2] = slot[0];                 // goes on from an earlier chunk: that chunk's thread of k14_stitch adds it
        else if (s == tail_slot && tail_out) a.part[(size_t)c * 2 + 1] = slot[s];
        else k14_store(a, v, slot[s]);
    }
    if (t == 0) a.meta[c] = make_uint2(tail_out ? sgrp[tail_slot] : SG_NONE, tail_out ? (K14_TAIL_OUT | (tail_slot == 0 ? K14_THROUGH : 0u)) : 0u);
}

__global__ __launch_bounds__(K14_THREADS) void k14_stitch(GroupArgs a) {
    const u64 E = k14_rows_of(a);
    const u32 C = (u32)((E + K14_CHUNK - 1) / K14_CHUNK);
    for (u32 c = blockIdx.x * K14_THREADS + threadIdx.x; c < C; c += gridDim.x * K14_THREADS) {
        const uint2 m = a.meta[c];
        if (!(m.y & K14_TAIL_OUT) || (m.y & K14_THROUGH)) continue;  // no run begins here and goes on
        K14Acc acc = a.part[(size_t)c * 2 + 1];
        for (u32 d = c + 1; d < C; d++) {
            k14_merge(acc, a.part[(size_t)d * 2]);
            if (!(a.meta[d].y & K14_THROUGH)) break;
        }
        k14_store(a, m.x, acc);
    }
}
