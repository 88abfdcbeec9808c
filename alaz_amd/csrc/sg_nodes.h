// sg_nodes.h — K9: the window's scored edges rolled up per node on the device (include/servicegraph.h, "node rollup").
// Part of the kernel translation unit: included last by sg_kernels.h.
//
// A node is keyed by idx = v (KNOWN), max_known + v (LABEL), max_known + max_labels + v (OBIP) with v = SG_REF_VALUE(ref): below
// ncap for every window, ascending in (type, value), and monotone in the dense numbering the rows are sorted by.  Every field is an
// integer sum, an integer max or the max of a 64-bit key — (order-preserving score key << 32 | ~row): the largest score, the
// smallest row among equal ones — so nothing depends on the order in which workgroups or lanes fold their parts in.  Five launches:
//
//   k9_out      out side: chunks of K9_CHUNK rows, each thread a span of K9_ROWS consecutive rows.  The rows are sorted by the
//               source's node, so a node's out rows are one run.  A run inside a thread's span is stored by that thread; a run cut
//               by a span boundary is folded into an LDS slot named by the first span boundary it crosses; a slot's run that stays
//               inside the chunk is stored by one thread, the (at most two) runs cut by the chunk's ends are added to the node with
//               device-scope integer atomics — two per chunk at most, never one per row, and a hub is never walked by one thread.
//               Beside it: the destination's node per row (dst), so the in side reads 4 bytes per row to find its rows.
//   k9_in_part  in side, k3_in_part's pattern: workgroup (range, slice) holds K9_IN_NR nodes in LDS, scans its slice of dst and
//               fetches the fields of the rows whose destination is in its range only; it writes its LDS to a per-slice partial.
//   k9_count    per node: the slices' partials summed into the in table; nodes with rows counted per workgroup
//   k9_scan     (1 workgroup) exclusive scan of the counts; the node count of the window
//   k9_write    the node rows in index order; the out table entries it read are zeroed for the next window (the out side adds to
//               them).  The tables are scratch shared by every window slot: launches on different streams are chained.
#pragma once

#define K9_THREADS 256            // k9_out, k9_count, k9_write
#define K9_ROWS 8                 // rows per thread of k9_out
#define K9_CHUNK (K9_THREADS * K9_ROWS)
#define K9_IN_THREADS 1024        // k9_in_part
#define K9_IN_NR 2048             // nodes per range: 2048 x 64 B = 128 KiB of LDS
#define K9_IN_Q 4                 // rows per thread and trip of k9_in_part
#define K9_SCAN_THREADS 1024      // k9_scan scans one count per thread
#define K9_MAX_WGS 1024

// one side of a node: sums, maxima, the worst-row key; 64 bytes (one LDS entry, one partial, one table entry)
struct K9Side { u64 cnt, err, sum, ssq, max, q32, worst; u32 edges, alive; };
static_assert(sizeof(K9Side) == 64, "K9Side is four 16-byte words");
static_assert(sizeof(sg_node_out) == 136 && offsetof(sg_node_out, ref) == 96 && offsetof(sg_node_out, out_score_max) == 124, "sg_node_out layout");

struct NodesArgs {
    const sg_edge_out* rows;      // the window's rows (canonical order)
    const u64* ctr;               // the window's counters: E = ctr[C_N_EDGES], and the used id ranges
    u64 max_edges;
    u32 mk, ml, mob, ncap;        // max_known, max_labels, max_obip; ncap = their sum
    u32 slices;                   // row slices of k9_in_part
    u32 node_per;                 // nodes per workgroup of k9_count / k9_write (a multiple of K9_THREADS)
    u32* dst;                     // [max_edges] node of each row's destination
    K9Side* tout;                 // [ncap] out side (zero between windows)
    K9Side* tin;                  // [ncap] in side (rewritten by k9_count)
    K9Side* part;                 // [ranges][slices][K9_IN_NR] per-slice in-side partials
    u32* blk;                     // [2][node workgroups]: nodes with rows, then their exclusive scan
    sg_node_out* out;             // [ncap] this window's node rows
    u64* count;                   // this window's node count
};

// order-preserving key of a float (+0.0 above -0.0) and back
__device__ __forceinline__ u32 k9_score_key(float s) { const u32 b = __float_as_uint(s); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float k9_key_score(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ u32 k9_node(const NodesArgs& a, u32 ref) {
    const u32 t = SG_REF_TYPE(ref), v = SG_REF_VALUE(ref);
    if (t == SG_REF_KNOWN) return v < a.mk ? v : SG_NONE;
    if (t == SG_REF_LABEL) return v < a.ml ? a.mk + v : SG_NONE;
    if (t == SG_REF_OBIP) return v < a.mob ? a.mk + a.ml + v : SG_NONE;
    return SG_NONE;
}
__device__ __forceinline__ u32 k9_ref(const NodesArgs& a, u32 v) {
    if (v < a.mk) return SG_MAKE_REF(SG_REF_KNOWN, v);
    if (v < a.mk + a.ml) return SG_MAKE_REF(SG_REF_LABEL, v - a.mk);
    return SG_MAKE_REF(SG_REF_OBIP, v - a.mk - a.ml);
}
// the node ids this window can hold: [0, nk), [mk, mk + nl), [mk + ml, mk + ml + nob)
struct K9Used { u32 a1, b0, b1, c0, c1; };
__device__ __forceinline__ K9Used k9_used(const NodesArgs& a) {
    const u64 nk = a.ctr[C_N_KNOWN], nl = a.ctr[C_N_LABELS], nob = a.ctr[C_N_OBIP];
    K9Used u;
    u.a1 = (u32)(nk < a.mk ? nk : a.mk);
    u.b0 = a.mk; u.b1 = a.mk + (u32)(nl < a.ml ? nl : a.ml);
    u.c0 = a.mk + a.ml; u.c1 = u.c0 + (u32)(nob < a.mob ? nob : a.mob);
    return u;
}
__device__ __forceinline__ bool k9_in_used(const K9Used& u, u32 v) { return v < u.a1 || (v >= u.b0 && v < u.b1) || (v >= u.c0 && v < u.c1); }
__device__ __forceinline__ bool k9_range_used(const K9Used& u, u32 n0, u32 n1) {   // [n0, n1) meets one of them
    return (n0 < u.a1) || (n0 < u.b1 && n1 > u.b0) || (n0 < u.c1 && n1 > u.c0);
}
// the window's node rows: its node count, at most the capacity (K11 - K13 walk the rows K9 wrote)
__device__ __forceinline__ u64 sg_nodes_of(const u64* count, u32 ncap) { const u64 N = *count; return N < ncap ? N : (u64)ncap; }
__device__ __forceinline__ u64 k9_rows_of(const NodesArgs& a) { const u64 E = a.ctr[C_N_EDGES]; return E < a.max_edges ? E : a.max_edges; }

// what a side needs of a row
struct K9Row { u64 sum, max, ssq; u32 from, to, cnt, err, alive; float score; };
__device__ __forceinline__ K9Row k9_load(const NodesArgs& a, u64 j) {
    const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.rows + j);    // words 0..7 (sg_k5.h)
    const ulonglong2 w01 = r[0], w23 = r[1], w45 = r[2], w67 = r[3];
    K9Row o;
    o.sum = w01.x; o.max = w01.y; o.ssq = w23.x;
    o.from = (u32)w23.y; o.to = (u32)(w23.y >> 32);
    o.cnt = (u32)w45.x; o.err = (u32)(w45.x >> 32);
    o.score = __uint_as_float((u32)w45.y);
    o.alive = (u32)(w67.x >> 32);
    return o;
}
__device__ __forceinline__ u64 k9_q32(float s) { return s > 0.0f ? (u64)((double)s * 4294967296.0) : 0ull; }
__device__ __forceinline__ u64 k9_worst_key(float s, u64 j) { return ((u64)k9_score_key(s) << 32) | (u64)(~(u32)j); }
__device__ __forceinline__ void k9_zero(K9Side& s) { s.cnt = s.err = s.sum = s.ssq = s.max = s.q32 = s.worst = 0; s.edges = s.alive = 0; }
__device__ __forceinline__ void k9_add(K9Side& s, const K9Row& r, u64 j) {
    s.edges += 1u; s.alive += r.alive; s.cnt += r.cnt; s.err += r.err; s.sum += r.sum; s.ssq += r.ssq;
    s.max = r.max > s.max ? r.max : s.max;
    s.q32 += k9_q32(r.score);
    const u64 k = k9_worst_key(r.score, j);
    s.worst = k > s.worst ? k : s.worst;
}
__device__ __forceinline__ void k9_merge(K9Side& s, const K9Side& o) {
    s.edges += o.edges; s.alive += o.alive; s.cnt += o.cnt; s.err += o.err; s.sum += o.sum; s.ssq += o.ssq; s.q32 += o.q32;
    s.max = o.max > s.max ? o.max : s.max;
    s.worst = o.worst > s.worst ? o.worst : s.worst;
}
// p may point to LDS or to global memory: the atomics are order-free integer adds and maxima
__device__ __forceinline__ void k9_atomic_merge(K9Side* p, const K9Side& o) {
    atomicAdd(&p->edges, o.edges);
    if (o.alive) atomicAdd(&p->alive, o.alive);
    atomicAdd(&p->cnt, o.cnt);
    if (o.err) atomicAdd(&p->err, o.err);
    atomicAdd(&p->sum, o.sum); atomicAdd(&p->ssq, o.ssq); atomicAdd(&p->q32, o.q32);
    atomicMax(&p->max, o.max); atomicMax(&p->worst, o.worst);
}
__device__ __forceinline__ void k9_store(K9Side* p, const K9Side& s) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(s.cnt, s.err); q[1] = make_ulonglong2(s.sum, s.ssq); q[2] = make_ulonglong2(s.max, s.q32);
    q[3] = make_ulonglong2(s.worst, (u64)s.edges | ((u64)s.alive << 32));
}
__device__ __forceinline__ K9Side k9_fetch(const K9Side* p) {
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
    K9Side s;
    s.cnt = x0.x; s.err = x0.y; s.sum = x1.x; s.ssq = x1.y; s.max = x2.x; s.q32 = x2.y; s.worst = x3.x;
    s.edges = (u32)x3.y; s.alive = (u32)(x3.y >> 32);
    return s;
}

// exclusive max over the workgroup's threads (values >= 0); wmax: LDS [NT / 64]
template <int NT>
__device__ __forceinline__ u32 k9_block_excl_max(u32 v, u32* wmax) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const u32 o = __shfl_up(incl, s, 64); if ((int)lane >= s) incl = o > incl ? o : incl; }
    u32 ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) wmax[wave] = incl;
    __syncthreads();
    for (u32 w = 0; w < wave; w++) ex = wmax[w] > ex ? wmax[w] : ex;
    return ex;
}

__global__ __launch_bounds__(K9_THREADS) void k9_out(NodesArgs a) {
    // slot b: the run whose first crossed span boundary is b (0 = the chunk's start: a run that began in an earlier chunk)
    __shared__ K9Side slot[K9_THREADS + 1];
    __shared__ u32 snode[K9_THREADS + 1];
    __shared__ u32 wmax[K9_THREADS / 64];
    __shared__ u32 tail_slot, tail_out;
    const u64 E = k9_rows_of(a);
    const u64 c0 = (u64)blockIdx.x * K9_CHUNK;
    if (c0 >= E) return;                                             // (uniform)
    const u64 c1 = c0 + K9_CHUNK < E ? c0 + K9_CHUNK : E;
    const u32 t = threadIdx.x;
    for (u32 s = t; s <= K9_THREADS; s += K9_THREADS) { k9_zero(slot[s]); snode[s] = SG_NONE; }
    const u64 j0 = c0 + (u64)t * K9_ROWS;
    const u32 n = j0 < c1 ? (u32)((c1 - j0) < K9_ROWS ? (c1 - j0) : K9_ROWS) : 0u;
    const u64 j1 = j0 + n;
    K9Row r[K9_ROWS];
    u32 f[K9_ROWS];
#pragma unroll
    for (int q = 0; q < K9_ROWS; q++) {
        if ((u32)q < n) {
            r[q] = k9_load(a, j0 + q);
            f[q] = k9_node(a, r[q].from);
            a.dst[j0 + q] = k9_node(a, r[q].to);
        } else {
            f[q] = SG_NONE;
        }
    }
    const u32 fprev = (n && j0 > 0) ? k9_node(a, (u32)reinterpret_cast<const u64*>(a.rows + j0 - 1)[3]) : SG_NONE;
    const u32 fnext = (n && j1 < E) ? k9_node(a, (u32)reinterpret_cast<const u64*>(a.rows + j1)[3]) : SG_NONE;
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
            if (!cut) { k9_store(a.tout + cur, acc); return; }       // the whole run is in this span: its only writer
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
            k9_add(acc, r[q], j0 + q);
        }
        const bool flows = j1 < E && fnext == cur;                   // the last run goes on past this span
        fold(flows || !here, here ? t + 1 : slot_first);
        if (j1 == c1) { tail_slot = here ? t + 1 : slot_first; tail_out = flows ? 1u : 0u; }
    }
    __syncthreads();
    for (u32 s = t; s <= K9_THREADS; s += K9_THREADS) {
        const u32 v = snode[s];
        if (v == SG_NONE) continue;
        if (s == 0 || (s == tail_slot && tail_out)) k9_atomic_merge(a.tout + v, slot[s]);   // shared with a neighbouring chunk
        else k9_store(a.tout + v, slot[s]);
    }
}

__global__ __launch_bounds__(K9_IN_THREADS) void k9_in_part(NodesArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    K9Side* acc = reinterpret_cast<K9Side*>(smem);
    const u32 S = a.slices, g = blockIdx.x, t = threadIdx.x;
    const u32 rg = g / S, sl = g % S, n0 = rg * K9_IN_NR;
    if (n0 >= a.ncap) return;
    const u32 nr = a.ncap - n0 < K9_IN_NR ? a.ncap - n0 : K9_IN_NR;
    if (!k9_range_used(k9_used(a), n0, n0 + nr)) return;            // (k9_count reads no partial of such a range)
    for (u32 i = t; i < nr; i += K9_IN_THREADS) k9_zero(acc[i]);
    __syncthreads();
    const u64 E = k9_rows_of(a);
    const u64 per = (E + S - 1) / S, p0 = (u64)sl * per < E ? (u64)sl * per : E, p1 = p0 + per < E ? p0 + per : E;
    // K9_IN_Q rows per thread and trip; the destinations of the next trip are fetched before this trip's rows
    u32 nxt[K9_IN_Q];
#pragma unroll
    for (int q = 0; q < K9_IN_Q; q++) { const u64 p = p0 + t + (u64)q * K9_IN_THREADS; nxt[q] = p < p1 ? a.dst[p] - n0 : 0xFFFFFFFFu; }
    for (u64 pb = p0 + t; pb < p1; pb += (u64)K9_IN_THREADS * K9_IN_Q) {
        u32 to[K9_IN_Q];
        K9Row x[K9_IN_Q];
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) { to[q] = nxt[q]; if (to[q] < nr) x[q] = k9_load(a, pb + (u64)q * K9_IN_THREADS); }
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) { const u64 p = pb + (u64)(K9_IN_Q + q) * K9_IN_THREADS; nxt[q] = p < p1 ? a.dst[p] - n0 : 0xFFFFFFFFu; }
#pragma unroll
        for (int q = 0; q < K9_IN_Q; q++) if (to[q] < nr) {
            K9Side* o = acc + to[q];
            const K9Row& y = x[q];
            atomicAdd(&o->edges, 1u);
            if (y.alive) atomicAdd(&o->alive, y.alive);
            atomicAdd(&o->cnt, (u64)y.cnt);
            if (y.err) atomicAdd(&o->err, (u64)y.err);
            atomicAdd(&o->sum, y.sum); atomicAdd(&o->ssq, y.ssq); atomicAdd(&o->q32, k9_q32(y.score));
            atomicMax(&o->max, y.max); atomicMax(&o->worst, k9_worst_key(y.score, pb + (u64)q * K9_IN_THREADS));
        }
    }
    __syncthreads();
    K9Side* out = a.part + ((size_t)rg * S + sl) * K9_IN_NR;
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(acc);
    ulonglong2* dp = reinterpret_cast<ulonglong2*>(out);
    for (u32 i = t; i < nr * 4; i += K9_IN_THREADS) dp[i] = src[i];
}

// the workgroup's nodes [v0, v1) in rounds of K9_THREADS
__device__ __forceinline__ void k9_node_span(const NodesArgs& a, u32& v0, u32& v1) {
    v0 = blockIdx.x * a.node_per; v1 = v0 + a.node_per;
    if (v0 > a.ncap) v0 = a.ncap;
    if (v1 > a.ncap) v1 = a.ncap;
}

__global__ __launch_bounds__(K9_THREADS) void k9_count(NodesArgs a) {
    __shared__ u32 ws[K9_THREADS / 64];
    const u32 t = threadIdx.x, S = a.slices;
    const K9Used u = k9_used(a);
    u32 v0, v1; k9_node_span(a, v0, v1);
    u32 c = 0;
    for (u32 v = v0 + t; v < v1; v += K9_THREADS) {
        K9Side in; k9_zero(in);
        if (k9_in_used(u, v)) {
            const u32 rg = v / K9_IN_NR, i = v - rg * K9_IN_NR;
            const K9Side* p = a.part + (size_t)rg * S * K9_IN_NR + i;
            for (u32 sl = 0; sl < S; sl++) k9_merge(in, k9_fetch(p + (size_t)sl * K9_IN_NR));
        }
        k9_store(a.tin + v, in);
        const u32 oe = reinterpret_cast<const u32*>(a.tout + v)[14];   // (out edges: word 14 of the entry)
        c += (oe + in.edges) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if ((t & 63) == 0) ws[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        u32 k = 0;
        for (int w = 0; w < K9_THREADS / 64; w++) k += ws[w];
        a.blk[blockIdx.x] = k;
    }
}

__global__ __launch_bounds__(K9_SCAN_THREADS) void k9_scan(NodesArgs a, u32 nwg) {
    __shared__ u32 wsum[K9_SCAN_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    const u32 c = t < nwg ? a.blk[t] : 0u;
    u32 tot;
    const u32 x = block_excl_scan<K9_SCAN_THREADS>(c, wsum, &tot);
    if (t < nwg) a.blk[K9_MAX_WGS + t] = x;
    if (t == 0) *a.count = tot;
}

__global__ __launch_bounds__(K9_THREADS) void k9_write(NodesArgs a) {
    __shared__ u32 wsum[K9_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    u32 v0, v1; k9_node_span(a, v0, v1);
    u32 base = a.blk[K9_MAX_WGS + blockIdx.x];
    for (u32 vb = v0; vb < v1; vb += K9_THREADS) {                  // (uniform: every thread takes every round)
        const u32 v = vb + t;
        K9Side O, I;
        bool has = false;
        if (v < v1) { O = k9_fetch(a.tout + v); I = k9_fetch(a.tin + v); has = (O.edges + I.edges) != 0; }
        u32 tot;
        const u32 x = block_excl_scan<K9_THREADS>(has ? 1u : 0u, wsum, &tot);
        if (has) {
            sg_node_out o;
            o.out_count = O.cnt; o.in_count = I.cnt; o.out_err = O.err; o.in_err = I.err;
            o.out_sum_ns = O.sum; o.in_sum_ns = I.sum; o.out_sumsq_us = O.ssq; o.in_sumsq_us = I.ssq;
            o.out_max_ns = O.max; o.in_max_ns = I.max; o.out_score_q32 = O.q32; o.in_score_q32 = I.q32;
            o.ref = k9_ref(a, v); o.out_edges = O.edges; o.in_edges = I.edges; o.out_alive = O.alive; o.in_alive = I.alive;
            o.out_worst_row = O.edges ? ~(u32)O.worst : 0xFFFFFFFFu; o.in_worst_row = I.edges ? ~(u32)I.worst : 0xFFFFFFFFu;
            o.out_score_max = O.edges ? k9_key_score((u32)(O.worst >> 32)) : 0.0f;
            o.in_score_max = I.edges ? k9_key_score((u32)(I.worst >> 32)) : 0.0f;
            o.score = o.out_score_max > o.in_score_max ? o.out_score_max : o.in_score_max;
            a.out[base + x] = o;
            if (O.edges) { K9Side z; k9_zero(z); k9_store(a.tout + v, z); }   // the out side adds into a zero table
        }
        base += tot;
    }
}
