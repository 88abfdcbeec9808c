// sg_node_trend.h — K10: per-node latency / error baselines kept across windows on the device, and the node selection
// (include/servicegraph.h, "node baselines").  Included after sg_sel.h and sg_trend.h: it reuses their helpers and two of their
// kernels unchanged (k8_scan, and K7's pick / count / scan / scatter / sort), and adds kernels of its own beside them.
//
// A window's node rows (K9) are strictly ascending by ref, i.e. by (type, value), and the outbound-IP list is ascending, so node key
// nk = type << 32 | x (x the value, the IPv4 address for OBIP refs: k8_ref_key) is strictly ascending too.  Each node row gives two
// samples, sample j = 2 * node + side with key (nk, side), side 0 = in, side 1 = out: the window's 2N samples are a sorted list and
// the update is K8's merge of the old entries with them — K8's own walk (sg_trend.h), over the sample source K10Nodes below:
//
//   k10_count  K8's count pass: merge-path split of the diagonal, one span per thread; the walk writes every sample's half of its
//              node's sg_node_trend (it needs only the prior entry) and counts the kept old entries and the new ones
//   k8_scan    (1 workgroup, K8's kernel on the TrendArgs part) scans, the capacity cut, the new B and the statistics
//   k10_write  K8's write pass: merged, updated, unexpired entries into the other buffer, in key order
//
// A side with count 0 (a pure caller has no in side) is a sample that neither creates nor refreshes an entry, as K8's alive-only rows.
// Samples read only the fields of their side: count, err and sum_ns (words 1 - s, 3 - s, 5 - s of the 136-byte row) and ref.
//
// Node selection is K7 with a key pass of its own (k10_keys: the node's score or a value of its sg_node_trend) over a count the key
// pass copies to word C_N_EDGES of a small counter block; K7's passes then select indices only (their row copies are off), and
// k_gather_sel<sg_node_out> (sg_kernels.h) copies the selected node rows.  No K7 or K8 kernel changes.
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

// sample j's side of its node's trend row: lat_dev, err_dev at words 2s, 2s + 1; base_mean_us at 4 + s; seen at 6 + s (the other
// side is another sample's: the two may be written by two threads, never the same bytes)
__device__ __forceinline__ void k10_put(sg_node_trend* out, u64 j, float ld, float ed, float base, u32 seen) {
    u32* w = reinterpret_cast<u32*>(out + (j >> 1));
    const u32 s = (u32)(j & 1u);
    w[2 * s] = __float_as_uint(ld); w[2 * s + 1] = __float_as_uint(ed); w[4 + s] = __float_as_uint(base); w[6 + s] = seen;
}

// K10's sample source for K8's walk: the window's 2 min(count, ncap) node samples, half an sg_node_trend each
struct K10Nodes {
    typedef NodeTrendArgs Args;
    typedef K10Sample Sample;
    static __device__ __forceinline__ u64 count(const NodeTrendArgs& a, u64) { const u64 N = *a.count; return 2 * (N < a.ncap ? N : (u64)a.ncap); }
    static __device__ __forceinline__ K10Sample sample(const NodeTrendArgs& a, u64 j, u32 nob) { return k10_sample(a, j, nob); }
    static __device__ __forceinline__ double x_lat(const K10Sample& r) { return k10_x_lat(r); }
    static __device__ __forceinline__ double x_err(const K10Sample& r) { return k10_x_err(r); }
    static __device__ __forceinline__ void put(const NodeTrendArgs& a, u64 j, float ld, float ed, float base, u32 seen) {
        k10_put(a.out, j, ld, ed, base, seen);
    }
};

__global__ __launch_bounds__(K8_THREADS) void k10_count(NodeTrendArgs na) { k8_count_t<K10Nodes, false>(na.t, na, VanArgs{}); }
__global__ __launch_bounds__(K8_THREADS) void k10_write(NodeTrendArgs na) { k8_write_t<K10Nodes, false>(na.t, na, VanArgs{}); }

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
