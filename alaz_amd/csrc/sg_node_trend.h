// sg_node_trend.h — K10: per-node latency / error baselines kept across windows on the device, and the node selection
// (include/servicegraph.h, "node baselines").  Included after sg_sel.h and sg_trend.h: it reuses their helpers and two of their
// kernels unchanged (k8_scan, and K7's pick / count / scan / scatter / sort), and adds kernels of its own beside them.
//
// A window's node rows (K9) are strictly ascending by ref, i.e. by (type, value), and the outbound-IP list is ascending, so node key
// nk = type << 32 | x (x the value, the IPv4 address for OBIP refs: k8_ref_key) is strictly ascending too.  Each node row gives two
// samples, sample j = 2 * node + side with key (nk, side), side 0 = in, side 1 = out: the window's 2N samples are a sorted list and
// the update is K8's merge of the old entries with them, word for word:
//
//   k10_count  merge-path split of the diagonal, one span per thread; the walk writes every sample's half of its node's
//              sg_node_trend (it needs only the prior entry) and counts the kept old entries and the new ones
//   k8_scan    (1 workgroup, K8's kernel on the TrendArgs part) scans, the capacity cut, the new B and the statistics
//   k10_write  the same walk again: merged, updated, unexpired entries into the other buffer, in key order
//
// A side with count 0 (a pure caller has no in side) is a sample that neither creates nor refreshes an entry, as K8's alive-only rows.
// Samples read only the fields of their side: count, err and sum_ns (words 1 - s, 3 - s, 5 - s of the 136-byte row) and ref.
//
// Node selection is K7 with a key pass of its own (k10_keys: the node's score or a value of its sg_node_trend) over a count the key
// pass copies to word C_N_EDGES of a small counter block; K7's passes then select indices only (their row copies are off), and
// k10_gather_rows copies the selected node rows.  No K7 or K8 kernel changes.
#pragma once

struct NodeTrendArgs {
    TrendArgs t;                  // K8's part: ctr (C_N_OBIP), ob_sorted, max_obip, cap, buf, th, blk, ctl, w, warmup, ttl, alpha, floors
    const sg_node_out* nodes;     // the window's node rows (K9, ascending by ref)
    const u64* count;             // their count
    u32 ncap;                     // the node rows a window can have
    sg_node_trend* out;           // [ncap] this window's node trend rows
};

// one sample: node j >> 1, side j & 1 (0 = in, 1 = out)
struct K10Sample { K8Key k; u64 sum, count, err; };
__device__ __forceinline__ K10Sample k10_sample(const NodeTrendArgs& a, u64 j, u32 nob) {
    const u64* r = reinterpret_cast<const u64*>(a.nodes + (j >> 1));  // words: 0 / 1 counts, 2 / 3 errors, 4 / 5 sum_ns (out / in)
    const u32 s = (u32)(j & 1u);
    K10Sample o;
    o.count = r[1 - s]; o.err = r[3 - s]; o.sum = r[5 - s];
    o.k.f = k8_ref_key(reinterpret_cast<const u32*>(r)[24], a.t.ob_sorted, nob);   // ref: byte 96
    o.k.t = s;
    return o;
}

// the per-window samples, exact in fp64: min(sum / count, 2^52) and floor(err * 2^20 / count) by long division (no overflow: the
// quotient's integer part err / count is shifted, the remainder's 20 fraction bits are found one at a time)
__device__ __forceinline__ double k10_x_lat(const K10Sample& r) {
    u64 m = r.sum / r.count;
    if (m > (1ull << 52)) m = 1ull << 52;
    return (double)m;
}
__device__ __forceinline__ double k10_x_err(const K10Sample& r) {
    const u64 c = r.count;
    u64 q = r.err / c, rem = r.err % c;
    for (int b = 0; b < 20; b++) {
        const u64 hi = rem >> 63;
        rem <<= 1;
        q <<= 1;
        if (hi || rem >= c) { rem -= c; q |= 1u; }
    }
    return (double)q;
}

struct K10Geom { u64 B, E; u32 nob; const TrendSoA* old; TrendSoA* nw; u32 par; };
__device__ __forceinline__ K10Geom k10_geom(const NodeTrendArgs& a) {
    K10Geom g;
    g.par = a.t.w & 1u;
    g.B = a.t.ctl[K8C_B0 + (g.par ^ 1u)];
    const u64 N = *a.count;
    g.E = 2 * (N < a.ncap ? N : (u64)a.ncap);
    const u64 nob = a.t.ctr[C_N_OBIP];
    g.nob = (u32)(nob < a.t.max_obip ? nob : a.t.max_obip);
    g.old = &a.t.buf[g.par ^ 1u]; g.nw = const_cast<TrendSoA*>(&a.t.buf[g.par]);
    return g;
}

// sample j's side of its node's trend row: lat_dev, err_dev at words 2s, 2s + 1; base_mean_us at 4 + s; seen at 6 + s (the other
// side is another sample's: the two may be written by two threads, never the same bytes)
__device__ __forceinline__ void k10_put(sg_node_trend* out, u64 j, float ld, float ed, float base, u32 seen) {
    u32* w = reinterpret_cast<u32*>(out + (j >> 1));
    const u32 s = (u32)(j & 1u);
    w[2 * s] = __float_as_uint(ld); w[2 * s + 1] = __float_as_uint(ed); w[4 + s] = __float_as_uint(base); w[6 + s] = seen;
}

// The walk of one thread's span (K8's k8_walk_t over samples).  WRITE = false: trend rows + counts; true: the merged entries.
template <bool WRITE>
__device__ __forceinline__ void k10_walk(const NodeTrendArgs& na, const K10Geom& g, u64 i, u64 j, u64 n, u32& kept, u32& fresh,
                                         u32& expired, u64 kb, u64 nb, u64 room) {
#pragma clang fp contract(off)
    const TrendArgs& a = na.t;
    const TrendSoA& A = *g.old;
    K8Key ak{}, pk{};                                   // the old entry at i, the one in front of it (i - 1)
    K10Sample r{};
    if (i < g.B) ak = k8_entry_key(A, i);
    if (i > 0) pk = k8_entry_key(A, i - 1);
    if (j < g.E) r = k10_sample(na, j, g.nob);
    for (u64 s = 0; s < n; s++) {
        if (i < g.B && (j >= g.E || k8_le(ak, r.k))) {  // an old entry
            const bool upd = j < g.E && r.count > 0 && k8_eq(ak, r.k);
            const u32 last = A.last[i];
            const bool keep = upd || a.w - last < a.ttl;
            if (keep) {
                if (WRITE) {
                    const u64 p = kb + (nb < room ? nb : room);
                    if (p < a.cap) {
                        TrendSoA& o = *g.nw;
                        double lm = A.lat_mean[i], ld = A.lat_dev[i], em = A.err_mean[i], ed = A.err_dev[i];
                        u32 cnt = A.n[i], ls = last;
                        if (upd) {
                            const double xl = k10_x_lat(r), xe = k10_x_err(r);
                            const double dl = xl - lm, de = xe - em;
                            lm = lm + dl * a.alpha; ld = ld + (fabs(dl) - ld) * a.alpha;
                            em = em + de * a.alpha; ed = ed + (fabs(de) - ed) * a.alpha;
                            cnt = cnt == 0xFFFFFFFFu ? cnt : cnt + 1u; ls = a.w;
                        }
                        o.from_key[p] = ak.f; o.to_key[p] = ak.t;
                        o.lat_mean[p] = lm; o.lat_dev[p] = ld; o.err_mean[p] = em; o.err_dev[p] = ed;
                        o.n[p] = cnt; o.last[p] = ls;
                    }
                }
                kb++; kept++;
            } else {
                expired++;
            }
            pk = ak; i++;
            if (i < g.B) ak = k8_entry_key(A, i);
        } else {                                        // a sample
            const bool match = i > 0 && k8_eq(pk, r.k);
            if (!WRITE) {
                float ld = 0.f, ed = 0.f, base = 0.f;
                u32 seen = 0;
                if (match) {
                    const u64 q = i - 1;
                    seen = A.n[q];
                    const double lm = A.lat_mean[q];
                    base = (float)(lm / 1000.0);
                    if (r.count > 0 && seen >= a.warmup) {
                        const double dd = A.lat_dev[q], em = A.err_mean[q], de = A.err_dev[q];
                        ld = (float)((k10_x_lat(r) - lm) / (dd > a.lat_floor ? dd : a.lat_floor));
                        ed = (float)((k10_x_err(r) - em) / (de > a.err_floor ? de : a.err_floor));
                    }
                }
                k10_put(na.out, j, ld, ed, base, seen);
            }
            if (!match && r.count > 0) {
                if (WRITE && nb < room) {
                    const u64 p = kb + nb;
                    if (p < a.cap) {
                        TrendSoA& o = *g.nw;
                        o.from_key[p] = r.k.f; o.to_key[p] = r.k.t;
                        o.lat_mean[p] = k10_x_lat(r); o.lat_dev[p] = 0.0; o.err_mean[p] = k10_x_err(r); o.err_dev[p] = 0.0;
                        o.n[p] = 1u; o.last[p] = a.w;
                    }
                }
                nb++; fresh++;
            }
            j++;
            if (j < g.E) r = k10_sample(na, j, g.nob);
        }
    }
}

__global__ __launch_bounds__(K8_THREADS) void k10_count(NodeTrendArgs na) {
    __shared__ u32 ws[3][K8_THREADS / 64];
    const TrendArgs& a = na.t;
    const u32 t = threadIdx.x;
    const K10Geom g = k10_geom(na);
    const u64 T = g.B + g.E;
    u64 d0, d1; k8_span(T, d0, d1);
    // merge path: how many old entries are among the first d0 merged elements (old first on equal keys)
    u64 lo = d0 > g.E ? d0 - g.E : 0, hi = d0 < g.B ? d0 : g.B;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (k8_le(k8_entry_key(*g.old, mid), k10_sample(na, d0 - 1 - mid, g.nob).k)) lo = mid + 1; else hi = mid;
    }
    u32 kept = 0, fresh = 0, expired = 0;
    k10_walk<false>(na, g, lo, d0 - lo, d1 - d0, kept, fresh, expired, 0, 0, 0);
    K8Thread& me = a.th[(size_t)blockIdx.x * K8_THREADS + t];
    me.i = lo; me.kept = kept; me.fresh = fresh;
    kept = wave_sum_u32(kept); fresh = wave_sum_u32(fresh); expired = wave_sum_u32(expired);
    if ((t & 63) == 0) { ws[0][t >> 6] = kept; ws[1][t >> 6] = fresh; ws[2][t >> 6] = expired; }
    __syncthreads();
    if (t == 0) {
        u32 k = 0, f = 0, x = 0;
        for (int w = 0; w < K8_THREADS / 64; w++) { k += ws[0][w]; f += ws[1][w]; x += ws[2][w]; }
        a.blk[(size_t)blockIdx.x * 4] = k; a.blk[(size_t)blockIdx.x * 4 + 1] = f; a.blk[(size_t)blockIdx.x * 4 + 2] = x;
    }
}

__global__ __launch_bounds__(K8_THREADS) void k10_write(NodeTrendArgs na) {
    __shared__ u32 wsum[K8_THREADS / 64 + 1];
    const TrendArgs& a = na.t;
    const u32 t = threadIdx.x;
    const K10Geom g = k10_geom(na);
    const u64 T = g.B + g.E;
    u64 d0, d1; k8_span(T, d0, d1);
    const K8Thread me = a.th[(size_t)blockIdx.x * K8_THREADS + t];
    u32 tot;
    const u32 kx = block_excl_scan<K8_THREADS>(me.kept, wsum, &tot);
    const u32 fx = block_excl_scan<K8_THREADS>(me.fresh, wsum, &tot);
    const u64 kb = (u64)a.blk[(size_t)blockIdx.x * 4 + 2] + kx, nb = (u64)a.blk[(size_t)blockIdx.x * 4 + 3] + fx;
    u32 kept = 0, fresh = 0, expired = 0;
    k10_walk<true>(na, g, me.i, d0 - me.i, d1 - d0, kept, fresh, expired, kb, nb, a.ctl[K8C_ROOM]);
}

// sg_window_node_trend with an index: the asked-for rows gathered on the device
__global__ __launch_bounds__(256) void k10_gather(const sg_node_trend* src, const u32* idx, u64 n, sg_node_trend* dst) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// ---- node selection ---------------------------------------------------------------------------------------------------------
// k7_keys over node rows: the key of the node's score (byte 132 of a 136-byte row) or of a value of its sg_node_trend (SG_NSEL_*:
// word by - 1 of 8), or for SG_NSEL_NEW one key for every node with in_seen == 0, out_seen == 0 and a request on either side.
// Workgroup 0 copies the node count to ctr[C_N_EDGES], where K7's later passes read it (a.ctr = ctr).
__global__ __launch_bounds__(K7_THREADS) void k10_keys(SelArgs a, const sg_node_out* nodes, const u64* count, const sg_node_trend* tr,
                                                       u32 by, u64* ctr) {
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
    const u32* tw = reinterpret_cast<const u32*>(tr);                      // 8 words per node trend row
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        u32 key;
        if (by == SG_NSEL_SCORE) {
            key = k7_key(nodes[i].score, a.min_score);
        } else if (by == SG_NSEL_NEW) {
            const uint2 seen = *reinterpret_cast<const uint2*>(tw + i * 8 + 6);
            const u64* r = reinterpret_cast<const u64*>(nodes + i);
            key = seen.x == 0u && seen.y == 0u && (r[0] | r[1]) != 0ull ? 0x80000000u : 0u;
        } else {
            key = k7_key(__uint_as_float(tw[i * 8 + (by - 1)]), a.min_score);
        }
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}

// the selected node rows: out[j] = nodes[idx[j]] for j < min(*n, cap)
__global__ __launch_bounds__(256) void k10_gather_rows(const sg_node_out* nodes, const u32* idx, const u64* n, u64 cap, sg_node_out* out) {
    const u64 m = *n < cap ? *n : cap;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256) out[j] = nodes[idx[j]];
}
