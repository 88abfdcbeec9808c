// sg_trend.h — K8: per-edge latency / error baselines kept across windows on the device (include/servicegraph.h, "trend").
//
// The baseline is a sorted array of entries (two SoA buffers, ping-pong by the parity of the trend-window counter w) and a window's
// rows are a sorted list too: the canonical row order (dense(from), dense(to)) is strictly ascending in the edge key (from_key,
// to_key).  A window's update is therefore a MERGE of the B old entries with the E rows — no hash table, no atomic insert:
//
//   k8_count   merge-path split of the diagonal, one span per thread; the walk writes every row's sg_edge_trend (it needs only
//              the prior entry) and counts the kept old entries and the new ones
//   k8_scan    (1 workgroup) exclusive scans of the per-workgroup counts, the capacity cut, the new B and the statistics
//   k8_write   the same walk again: merged, updated, unexpired entries into the other buffer, in key order
//
// Ties of the merge are taken from the old list first, so an entry and the row with its key are neighbours of the merged order,
// the entry first: a row looks back at the entry in front of it (its thread's split, or the last one its walk passed), an entry
// looks at the row behind it (the next row of the walk).  Each element decides alone, so a matched pair that straddles two spans
// needs nothing special.  Nothing depends on workgroup order and there are no global atomics: every count is reduced in order.
// The device control block keeps B per parity: window w reads buffer / B of parity (w - 1) & 1 and writes those of parity w & 1.
//
// The split, the walk, the scan and the write pass are one template body each (k8_count_t, k8_walk_t, k8_scan_t, k8_write_t),
// generic over a sample source: K8Edges here (the window's rows), K10Nodes in sg_node_trend.h (two samples per node row).  The
// count, scan and write kernels of K8 and K10 are one-line wrappers of them.
//
// Vanished dependencies (sg_set_vanished) ride on the same walk: k8_count_v / k8_scan_v / k8_write_v are the three bodies with VAN
// set, one more count.  An old entry the walk passes that is not refreshed, has seen min_seen windows and went without a sample for
// exactly silent windows is counted per thread and per workgroup, scanned, and written at its key-order position; the row behind it
// (the next row of the walk) is the window's alive-only row with its key, if there is one.  With the list off the plain kernels run.
#pragma once

#define K8_THREADS 256            // k8_count / k8_write
#define K8_SCAN_THREADS 1024      // k8_scan scans one count per thread
#define K8_MAX_WGS 1024

// control block (u64 words)
enum { K8C_B0 = 0, K8C_B1, K8C_ROOM, K8C_WINDOWS, K8C_INSERTED, K8C_EXPIRED, K8C_DROPPED, K8C_PAD, K8C_WORDS = 8 };

struct TrendSoA {
    u64* from_key; u64* to_key;
    double* lat_mean; double* lat_dev; double* err_mean; double* err_dev;
    u32* n; u32* last;
};

// per thread of k8_count: its split (old entries before its span) and its counts
struct K8Thread { u64 i; u32 kept, fresh; };

struct TrendArgs {
    const sg_edge_out* rows;      // the window's rows (canonical order)
    const u64* ctr;               // the window's counters: E = ctr[C_N_EDGES], outbound IPs = ctr[C_N_OBIP]
    const u32* ob_sorted;         // the window's ascending outbound-IP list
    u32 max_obip;
    u64 max_edges;
    u64 cap;                      // max_entries
    TrendSoA buf[2];
    sg_edge_trend* out;           // [max_edges] this window's trend rows
    K8Thread* th;                 // [wgs * K8_THREADS]
    u32* blk;                     // [wgs][4]: kept, new, expired -> kept before, new before (k8_scan)
    u64* ctl;                     // [K8C_WORDS]
    u32 w, warmup, ttl, pad;
    double alpha, lat_floor, err_floor;
};

// the vanished list of one window (sg_set_vanished): per slot the list and its count, the per-thread / per-workgroup counts scratch
struct VanArgs {
    sg_edge_vanished* out;        // [max_rows] the window slot's list
    u64* count;                   // the slot's count: every vanished entry of the window
    u32* th;                      // [wgs * K8_THREADS] per-thread counts (k8_count_v)
    u32* blk;                     // [wgs] per-workgroup counts -> vanished before (k8_scan_v)
    u64 max_rows;
    u32 silent, min_seen;
};

struct K8Key { u64 f, t; };
__device__ __forceinline__ bool k8_le(const K8Key& a, const K8Key& b) { return a.f < b.f || (a.f == b.f && a.t <= b.t); }
__device__ __forceinline__ bool k8_eq(const K8Key& a, const K8Key& b) { return a.f == b.f && a.t == b.t; }

// what the walk needs of a row: its key (OBIP refs through the outbound-IP list) and sum_ns / count / err_count
struct K8Row { K8Key k; u64 sum; u32 count, err; };
__device__ __forceinline__ u64 k8_ref_key(u32 ref, const u32* ob, u32 nob) {
    const u32 t = SG_REF_TYPE(ref), v = SG_REF_VALUE(ref);
    const u64 x = t == SG_REF_OBIP ? (v < nob ? (u64)ob[v] : 0ull) : (u64)v;
    return ((u64)t << 32) | x;
}
__device__ __forceinline__ K8Row k8_row(const TrendArgs& a, u64 j, u32 nob) {
    const u64* r = reinterpret_cast<const u64*>(a.rows + j);    // words 0 (sum_ns), 3 (from_ref | to_ref << 32), 4 (count | err_count << 32)
    const u64 s = r[0], refs = r[3], ce = r[4];
    K8Row o;
    o.k.f = k8_ref_key((u32)refs, a.ob_sorted, nob); o.k.t = k8_ref_key((u32)(refs >> 32), a.ob_sorted, nob);
    o.sum = s; o.count = (u32)ce; o.err = (u32)(ce >> 32);
    return o;
}
__device__ __forceinline__ K8Key k8_entry_key(const TrendSoA& b, u64 i) { K8Key k; k.f = b.from_key[i]; k.t = b.to_key[i]; return k; }

// the per-window samples: exact integers in fp64
__device__ __forceinline__ double k8_x_lat(const K8Row& r) {
    u64 m = r.sum / r.count;
    if (m > (1ull << 52)) m = 1ull << 52;
    return (double)m;
}
__device__ __forceinline__ double k8_x_err(const K8Row& r) { return (double)(((u64)r.err << 20) / r.count); }

// K8's sample source: the window's edge rows, E = ctr[C_N_EDGES] clamped to max_edges, one sg_edge_trend per row.  A source (K10's
// nodes are the other: sg_node_trend.h) names its kernel argument (Args; the passes take its TrendArgs part beside it) and its
// sample type, says how many samples the window has (count: given the window's edge counter, which k8_geom loads together with the
// outbound-IP counter next to it), reads sample j, finds x_lat / x_err of it and stores its trend output.
struct K8Edges {
    typedef TrendArgs Args;
    typedef K8Row Sample;
    static __device__ __forceinline__ u64 count(const TrendArgs& a, u64 edges) { return edges < a.max_edges ? edges : a.max_edges; }
    static __device__ __forceinline__ K8Row sample(const TrendArgs& a, u64 j, u32 nob) { return k8_row(a, j, nob); }
    static __device__ __forceinline__ double x_lat(const K8Row& r) { return k8_x_lat(r); }
    static __device__ __forceinline__ double x_err(const K8Row& r) { return k8_x_err(r); }
    static __device__ __forceinline__ void put(const TrendArgs& a, u64 j, float ld, float ed, float base, u32 seen) {
        sg_edge_trend t; t.lat_dev = ld; t.err_dev = ed; t.base_mean_us = base; t.windows_seen = seen;
        a.out[j] = t;
    }
};

struct K8Geom { u64 B, E; u32 nob; const TrendSoA* old; TrendSoA* nw; u32 par; };
template <class S>
__device__ __forceinline__ K8Geom k8_geom(const TrendArgs& a, const typename S::Args& sa) {
    K8Geom g;
    g.par = a.w & 1u;
    g.B = a.ctl[K8C_B0 + (g.par ^ 1u)];
    g.E = S::count(sa, a.ctr[C_N_EDGES]);
    const u64 nob = a.ctr[C_N_OBIP];
    g.nob = (u32)(nob < a.max_obip ? nob : a.max_obip);
    g.old = &a.buf[g.par ^ 1u]; g.nw = const_cast<TrendSoA*>(&a.buf[g.par]);
    return g;
}
// this thread's span [d0, d1) of the merged order
__device__ __forceinline__ void k8_span(u64 T, u64& d0, u64& d1) {
    const u64 nt = (u64)gridDim.x * K8_THREADS, per = (T + nt - 1) / nt;
    const u64 gt = (u64)blockIdx.x * K8_THREADS + threadIdx.x;
    d0 = gt * per; d1 = d0 + per;
    if (d0 > T) d0 = T;
    if (d1 > T) d1 = T;
}

// How the walk counts the old entries it keeps and expires.  Written as `if (keep) kept++; else expired++;` the compiler folds the
// two bumps into one indexed bump of a private array: 12 bytes of scratch a lane and two scratch accesses per old entry, in every
// instantiation without the vanished count.  A source that says flat_counts adds the two conditions instead and keeps the counters
// in registers (K21's, sg_quantile_trend.h).  K8, K10, K15 and K16 stay as they were measured: their code does not change.
template <class S, class = void> struct K8FlatCounts { static constexpr bool value = false; };
template <class S> struct K8FlatCounts<S, decltype((void)S::flat_counts)> { static constexpr bool value = S::flat_counts; };

// The walk of one thread's span over source S's samples, shared by both passes.  WRITE = false: trend rows + counts; true: the
// merged entries.  VAN (edges only): also count (and with WRITE write) the vanished entries: van counts them, vb = the position of
// this thread's first one.
template <class S, bool WRITE, bool VAN>
__device__ __forceinline__ void k8_walk_t(const TrendArgs& a, const typename S::Args& sa, const K8Geom& g, u64 i, u64 j, u64 n, u32& kept,
                                          u32& fresh, u32& expired, u64 kb, u64 nb, u64 room, const VanArgs& v, u32& van, u64 vb) {
#pragma clang fp contract(off)
    const TrendSoA& A = *g.old;
    K8Key ak{}, pk{};                                   // the old entry at i, the one in front of it (i - 1)
    typename S::Sample r{};
    if (i < g.B) ak = k8_entry_key(A, i);
    if (i > 0) pk = k8_entry_key(A, i - 1);
    if (j < g.E) r = S::sample(sa, j, g.nob);
    for (u64 s = 0; s < n; s++) {
        if (i < g.B && (j >= g.E || k8_le(ak, r.k))) {  // an old entry
            const bool upd = j < g.E && r.count > 0 && k8_eq(ak, r.k);
            const u32 last = A.last[i];
            const bool keep = upd || a.w - last < a.ttl;
            if (VAN && !upd && a.w - last == v.silent && A.n[i] >= v.min_seen) {   // (silent < ttl: kept, unchanged)
                if (WRITE) {
                    const u64 p = vb + van;
                    if (p < v.max_rows) {
                        sg_edge_vanished x;
                        x.from_key = ak.f; x.to_key = ak.t;
                        x.lat_mean = A.lat_mean[i]; x.lat_dev = A.lat_dev[i]; x.err_mean = A.err_mean[i]; x.err_dev = A.err_dev[i];
                        x.n = A.n[i]; x.last = last;
                        x.row = j < g.E && k8_eq(ak, r.k) ? (u32)j : 0xFFFFFFFFu;    // the row behind it: alive-only (upd is false)
                        x.reserved = 0;
                        v.out[p] = x;
                    }
                }
                van++;
            }
            if (keep) {
                if (WRITE) {
                    const u64 p = kb + (nb < room ? nb : room);
                    if (p < a.cap) {
                        TrendSoA& o = *g.nw;
                        double lm = A.lat_mean[i], ld = A.lat_dev[i], em = A.err_mean[i], ed = A.err_dev[i];
                        u32 cnt = A.n[i], ls = last;
                        if (upd) {
                            const double xl = S::x_lat(r), xe = S::x_err(r);
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
                kb++;
                if constexpr (!K8FlatCounts<S>::value) kept++;
            } else {
                if constexpr (!K8FlatCounts<S>::value) expired++;
            }
            if constexpr (K8FlatCounts<S>::value) { kept += keep ? 1u : 0u; expired += keep ? 0u : 1u; }
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
                        ld = (float)((S::x_lat(r) - lm) / (dd > a.lat_floor ? dd : a.lat_floor));
                        ed = (float)((S::x_err(r) - em) / (de > a.err_floor ? de : a.err_floor));
                    }
                }
                S::put(sa, j, ld, ed, base, seen);
            }
            if (!match && r.count > 0) {
                if (WRITE && nb < room) {
                    const u64 p = kb + nb;
                    if (p < a.cap) {
                        TrendSoA& o = *g.nw;
                        o.from_key[p] = r.k.f; o.to_key[p] = r.k.t;
                        o.lat_mean[p] = S::x_lat(r); o.lat_dev[p] = 0.0; o.err_mean[p] = S::x_err(r); o.err_dev[p] = 0.0;
                        o.n[p] = 1u; o.last[p] = a.w;
                    }
                }
                nb++; fresh++;
            }
            j++;
            if (j < g.E) r = S::sample(sa, j, g.nob);
        }
    }
}

// the count pass (k8_count, k8_count_v, k10_count): the merge-path split, the walk, the per-thread and per-workgroup counts
template <class S, bool VAN>
__device__ __forceinline__ void k8_count_t(const TrendArgs& a, const typename S::Args& sa, const VanArgs& v) {
    __shared__ u32 ws[VAN ? 4 : 3][K8_THREADS / 64];
    const u32 t = threadIdx.x;
    const K8Geom g = k8_geom<S>(a, sa);
    const u64 T = g.B + g.E;
    u64 d0, d1; k8_span(T, d0, d1);
    // merge path: how many old entries are among the first d0 merged elements (old first on equal keys)
    u64 lo = d0 > g.E ? d0 - g.E : 0, hi = d0 < g.B ? d0 : g.B;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (k8_le(k8_entry_key(*g.old, mid), S::sample(sa, d0 - 1 - mid, g.nob).k)) lo = mid + 1; else hi = mid;
    }
    u32 kept = 0, fresh = 0, expired = 0, van = 0;
    k8_walk_t<S, false, VAN>(a, sa, g, lo, d0 - lo, d1 - d0, kept, fresh, expired, 0, 0, 0, v, van, 0);
    K8Thread& me = a.th[(size_t)blockIdx.x * K8_THREADS + t];
    me.i = lo; me.kept = kept; me.fresh = fresh;
    if constexpr (VAN) v.th[(size_t)blockIdx.x * K8_THREADS + t] = van;
    kept = wave_sum_u32(kept); fresh = wave_sum_u32(fresh); expired = wave_sum_u32(expired);
    if constexpr (VAN) van = wave_sum_u32(van);
    if ((t & 63) == 0) {
        ws[0][t >> 6] = kept; ws[1][t >> 6] = fresh; ws[2][t >> 6] = expired;
        if constexpr (VAN) ws[3][t >> 6] = van;
    }
    __syncthreads();
    if (t == 0) {
        u32 k = 0, f = 0, x = 0, y = 0;
        for (int w = 0; w < K8_THREADS / 64; w++) {
            k += ws[0][w]; f += ws[1][w]; x += ws[2][w];
            if constexpr (VAN) y += ws[3][w];
        }
        a.blk[(size_t)blockIdx.x * 4] = k; a.blk[(size_t)blockIdx.x * 4 + 1] = f; a.blk[(size_t)blockIdx.x * 4 + 2] = x;
        if constexpr (VAN) v.blk[blockIdx.x] = y;
    }
}

// the scan (k8_scan, k8_scan_v; one workgroup): exclusive scans of the per-workgroup counts, the capacity cut (the kept old entries
// never exceed max_entries: the first max_entries - kept new ones in key order go in), the new B and the running statistics; VAN:
// the vanished counts scanned too, their per-workgroup base and the window's count
template <bool VAN>
__device__ __forceinline__ void k8_scan_t(const TrendArgs& a, u32 nwg, const VanArgs& v) {
    __shared__ u32 wsum[K8_SCAN_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    const u32 k = t < nwg ? a.blk[(size_t)t * 4] : 0u, f = t < nwg ? a.blk[(size_t)t * 4 + 1] : 0u, x = t < nwg ? a.blk[(size_t)t * 4 + 2] : 0u;
    u32 ktot, ftot, xtot;
    const u32 kb = block_excl_scan<K8_SCAN_THREADS>(k, wsum, &ktot);
    const u32 fb = block_excl_scan<K8_SCAN_THREADS>(f, wsum, &ftot);
    block_excl_scan<K8_SCAN_THREADS>(x, wsum, &xtot);
    if (t < nwg) { a.blk[(size_t)t * 4 + 2] = kb; a.blk[(size_t)t * 4 + 3] = fb; }
    if constexpr (VAN) {
        u32 vtot;
        const u32 y = t < nwg ? v.blk[t] : 0u;
        const u32 yb = block_excl_scan<K8_SCAN_THREADS>(y, wsum, &vtot);
        if (t < nwg) v.blk[t] = yb;
        if (t == 0) *v.count = vtot;
    }
    if (t == 0) {
        const u64 room = a.cap > ktot ? a.cap - ktot : 0ull;
        const u64 ins = ftot < room ? ftot : room;
        a.ctl[K8C_ROOM] = room;
        a.ctl[K8C_B0 + (a.w & 1u)] = ktot + ins;
        a.ctl[K8C_WINDOWS] += 1;
        a.ctl[K8C_INSERTED] += ins;
        a.ctl[K8C_EXPIRED] += xtot;
        a.ctl[K8C_DROPPED] += ftot - ins;
    }
}

// the write pass (k8_write, k8_write_v, k10_write): the walk again from the count pass's split, at the scanned positions; VAN: each
// vanished entry written at its key-order position
template <class S, bool VAN>
__device__ __forceinline__ void k8_write_t(const TrendArgs& a, const typename S::Args& sa, const VanArgs& v) {
    __shared__ u32 wsum[K8_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    const K8Geom g = k8_geom<S>(a, sa);
    const u64 T = g.B + g.E;
    u64 d0, d1; k8_span(T, d0, d1);
    const K8Thread me = a.th[(size_t)blockIdx.x * K8_THREADS + t];
    u32 tot;
    const u32 kx = block_excl_scan<K8_THREADS>(me.kept, wsum, &tot);
    const u32 fx = block_excl_scan<K8_THREADS>(me.fresh, wsum, &tot);
    const u64 kb = (u64)a.blk[(size_t)blockIdx.x * 4 + 2] + kx, nb = (u64)a.blk[(size_t)blockIdx.x * 4 + 3] + fx;
    u64 vb = 0;
    if constexpr (VAN) vb = (u64)v.blk[blockIdx.x] + block_excl_scan<K8_THREADS>(v.th[(size_t)blockIdx.x * K8_THREADS + t], wsum, &tot);
    u32 kept = 0, fresh = 0, expired = 0, van = 0;
    k8_walk_t<S, true, VAN>(a, sa, g, me.i, d0 - me.i, d1 - d0, kept, fresh, expired, kb, nb, a.ctl[K8C_ROOM], v, van, vb);
}

__global__ __launch_bounds__(K8_THREADS) void k8_count(TrendArgs a) { k8_count_t<K8Edges, false>(a, a, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k8_count_v(TrendArgs a, VanArgs v) { k8_count_t<K8Edges, true>(a, a, v); }
__global__ __launch_bounds__(K8_SCAN_THREADS) void k8_scan(TrendArgs a, u32 nwg) { k8_scan_t<false>(a, nwg, VanArgs{}); }
__global__ __launch_bounds__(K8_SCAN_THREADS) void k8_scan_v(TrendArgs a, u32 nwg, VanArgs v) { k8_scan_t<true>(a, nwg, v); }
__global__ __launch_bounds__(K8_THREADS) void k8_write(TrendArgs a) { k8_write_t<K8Edges, false>(a, a, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k8_write_v(TrendArgs a, VanArgs v) { k8_write_t<K8Edges, true>(a, a, v); }
