// sg_sel.h — K7: selection of a closed window's rows on the device (include/servicegraph.h, "selection").
//
// The rows sit on the device in canonical order with the score as an fp32 at byte 40 of each 64-byte row.  A selection moves rows,
// it computes nothing: every pass below is integer work on a 32-bit order-preserving key per row, and nothing depends on the order
// workgroups run in (per-workgroup LDS histograms and counts, reduced by one workgroup; no global atomics).
//
//   k7_keys     key of every row (0 = not a candidate) + per-workgroup histogram of the key's top byte
//   k7_keys_by  the same from the window's trend rows (sg_edge_trend: lat_dev / err_dev, or windows_seen == 0 with count > 0)
//   k7_pick     (1 workgroup) round r of the MSD radix select: which byte of the k-th largest key, how many above it
//   k7_hist     per-workgroup histogram of byte r among the keys that share the bytes picked so far (rounds 1..3)
//   k7_count    per workgroup: keys above the threshold key T, keys equal to T
//   k7_scan     (1 workgroup) their exclusive scans over the workgroups; the count selected
//   k7_scatter  ordered compaction: threshold mode writes the rows and indices, top-k mode (~key, index) pairs
//   k7_sort     (1 workgroup) top-k mode: the pairs sorted in LDS (key descending, index ascending), rows and indices gathered
//
// Tie rule: the keys above T are all selected, the keys equal to T in ascending row order until k are: element i goes to
// position gt_before(i) + min(eq_before(i), need) — two prefix counts, so the compaction needs no second pass.
#pragma once

#define K7_THREADS 256            // multi-workgroup passes
#define K7_PICK_THREADS 1024      // k7_pick / k7_scan / k7_sort
#define K7_MAX_WGS 1024           // k7_scan scans one count per thread

// k7 state words (u32)
enum { K7S_PREFIX = 0, K7S_REM, K7S_DONE, K7S_SEL, K7S_WORDS = 8 };

struct SelArgs {
    const sg_edge_out* rows;      // the window's rows
    const u64* ctr;               // the window's counters on the device (E = ctr[C_N_EDGES]), or null: E = n_host
    u64 n_host;
    u64 max_edges;                // E is clamped to it (the keys array's size)
    float min_score;
    u32 k;                        // 0 = threshold mode
    u32* keys;                    // [max_edges]
    u32* hist;                    // [workgroups][256]
    u32* blk;                     // [workgroups][4]: gt count, eq count, gt before, eq before
    u32* state;                   // [K7S_WORDS]
    u64* pairs;                   // [SG_SELECT_MAX_K]
    sg_edge_out* out;             // [cap] (may be null)
    u32* out_idx;                 // [cap] (may be null)
    u64 cap;
    u64* n_out;                   // rows selected (device)
};

__device__ __forceinline__ u64 k7_rows(const SelArgs& a) {
    const u64 E = a.ctr ? a.ctr[C_N_EDGES] : a.n_host;
    return E < a.max_edges ? E : a.max_edges;
}
// rows of workgroup b: [lo, hi), contiguous, in order of b (the compaction's order)
__device__ __forceinline__ void k7_span(u64 E, u64& lo, u64& hi) {
    const u64 nb = gridDim.x, per = (E + nb - 1) / nb;
    lo = (u64)blockIdx.x * per; hi = lo + per;
    if (lo > E) lo = E;
    if (hi > E) hi = E;
}
// order-preserving key of a candidate score: larger score, larger key; -0.0 and +0.0 the same key; every candidate key > 0
__device__ __forceinline__ u32 k7_key(float s, float min_score) {
    if (!(s >= min_score)) return 0u;
    u32 u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(K7_THREADS) void k7_keys(SelArgs a) {
    __shared__ u32 h[256];
    const u32 t = threadIdx.x;
    h[t] = 0;
    if (blockIdx.x == 0 && t == 0) {
        a.state[K7S_PREFIX] = 0; a.state[K7S_REM] = a.k; a.state[K7S_DONE] = a.k == 0 ? 1u : 0u; a.state[K7S_SEL] = 0;
    }
    __syncthreads();
    const u64 E = k7_rows(a);
    u64 lo, hi; k7_span(E, lo, hi);
    const float* sc = reinterpret_cast<const float*>(a.rows) + 10;          // score: byte 40 of a 64-byte row
    u64 i = lo + t;
    for (; i + 3 * K7_THREADS < hi; i += 4 * K7_THREADS) {                  // four rows in flight per lane
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = sc[(i + (u64)j * K7_THREADS) * 16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 key = k7_key(s[j], a.min_score);
            a.keys[i + (u64)j * K7_THREADS] = key;
            if (key && a.k) atomicAdd(&h[key >> 24], 1u);
        }
    }
    for (; i < hi; i += K7_THREADS) {
        const u32 key = k7_key(sc[i * 16], a.min_score);
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}

// k7_keys with the key of a trend value (SG_SEL_LAT_DEV: byte 0 of a 16-byte sg_edge_trend, SG_SEL_ERR_DEV: byte 4) or, for
// SG_SEL_NEW, one key for every new dependency (windows_seen == 0 and count > 0): ties by row position give the first k of them
__global__ __launch_bounds__(K7_THREADS) void k7_keys_by(SelArgs a, const sg_edge_trend* tr, u32 by) {
    __shared__ u32 h[256];
    const u32 t = threadIdx.x;
    h[t] = 0;
    if (blockIdx.x == 0 && t == 0) {
        a.state[K7S_PREFIX] = 0; a.state[K7S_REM] = a.k; a.state[K7S_DONE] = a.k == 0 ? 1u : 0u; a.state[K7S_SEL] = 0;
    }
    __syncthreads();
    const u64 E = k7_rows(a);
    u64 lo, hi; k7_span(E, lo, hi);
    const u32* tw = reinterpret_cast<const u32*>(tr);                      // 4 words per trend row
    const u32* cw = reinterpret_cast<const u32*>(a.rows) + 8;               // count: byte 32 of a 64-byte row
    const u32 off = by == SG_SEL_ERR_DEV ? 1u : 0u;
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        u32 key;
        if (by == SG_SEL_NEW) key = tw[i * 4 + 3] == 0u && cw[i * 16] > 0u ? 0x80000000u : 0u;
        else key = k7_key(__uint_as_float(tw[i * 4 + off]), a.min_score);
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}

// byte `round` (0 = top) of the keys whose higher bytes are the prefix picked so far
__global__ __launch_bounds__(K7_THREADS) void k7_hist(SelArgs a, u32 round) {
    if (a.state[K7S_DONE]) return;
    __shared__ u32 h[256];
    const u32 t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const u32 shift = 24 - 8 * round, hmask = ~0u << (32 - 8 * round), prefix = a.state[K7S_PREFIX];
    const u64 E = k7_rows(a);
    u64 lo, hi; k7_span(E, lo, hi);
    for (u64 i = lo + t; i < hi; i += K7_THREADS) {
        const u32 key = a.keys[i];
        if (key && (key & hmask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}

// one workgroup: sum the per-workgroup histograms, walk the bins from the top, fix byte `round` of the k-th largest key
__global__ __launch_bounds__(K7_PICK_THREADS) void k7_pick(SelArgs a, u32 round, u32 nwg) {
    if (a.state[K7S_DONE]) return;
    __shared__ u32 part[4][256];
    __shared__ u32 wsum[K7_PICK_THREADS / 64 + 1];
    const u32 t = threadIdx.x, bin = t & 255, q = t >> 8;
    u32 s = 0;
    for (u32 b = q; b < nwg; b += 4) s += a.hist[(size_t)b * 256 + bin];
    part[q][bin] = s;
    __syncthreads();
    // thread t < 256 takes bin 255 - t: the exclusive scan over threads is the count in the bins above
    const u32 d = 255 - (t & 255);
    const u32 c = t < 256 ? part[0][d] + part[1][d] + part[2][d] + part[3][d] : 0u;
    u32 total;
    const u32 above = block_excl_scan<K7_PICK_THREADS>(c, wsum, &total);
    const u32 rem = a.state[K7S_REM], prefix = a.state[K7S_PREFIX];
    __syncthreads();                                                        // every thread has read the state
    if (round == 0 && total <= rem) {                                       // all candidates fit: keys > 0
        if (t == 0) { a.state[K7S_PREFIX] = 0; a.state[K7S_REM] = 0; a.state[K7S_DONE] = 1; }
        return;
    }
    if (t < 256 && above < rem && above + c >= rem) {                       // exactly one bin
        const u32 shift = 24 - 8 * round;
        const u32 p = prefix | (d << shift);
        if (above + c == rem) {                                             // the whole bin is taken: keys >= p (> 0), no ties needed
            a.state[K7S_PREFIX] = p ? p - 1 : 0u; a.state[K7S_REM] = 0; a.state[K7S_DONE] = 1;
        } else {
            a.state[K7S_PREFIX] = p; a.state[K7S_REM] = rem - above;
            if (round == 3) a.state[K7S_DONE] = 1;                          // T = p, need = rem - above ties at T
        }
    }
}

// keys above T, keys equal to T, of this workgroup's rows (T = state[PREFIX], need = state[REM])
__global__ __launch_bounds__(K7_THREADS) void k7_count(SelArgs a) {
    __shared__ u32 ws[2][K7_THREADS / 64];
    const u32 t = threadIdx.x, T = a.state[K7S_PREFIX];
    const u64 E = k7_rows(a);
    u64 lo, hi; k7_span(E, lo, hi);
    u32 gt = 0, eq = 0;
    for (u64 i = lo + t; i < hi; i += K7_THREADS) { const u32 key = a.keys[i]; gt += key > T; eq += key == T; }
    gt = wave_sum_u32(gt); eq = wave_sum_u32(eq);
    if ((t & 63) == 0) { ws[0][t >> 6] = gt; ws[1][t >> 6] = eq; }
    __syncthreads();
    if (t == 0) {
        u32 g = 0, e = 0;
        for (int w = 0; w < K7_THREADS / 64; w++) { g += ws[0][w]; e += ws[1][w]; }
        a.blk[(size_t)blockIdx.x * 4] = g; a.blk[(size_t)blockIdx.x * 4 + 1] = e;
    }
}

// one workgroup: exclusive scans of the per-workgroup counts; the number selected
__global__ __launch_bounds__(K7_PICK_THREADS) void k7_scan(SelArgs a, u32 nwg) {
    __shared__ u32 wsum[K7_PICK_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    const u32 g = t < nwg ? a.blk[(size_t)t * 4] : 0u, e = t < nwg ? a.blk[(size_t)t * 4 + 1] : 0u;
    u32 gtot, etot;
    const u32 gb = block_excl_scan<K7_PICK_THREADS>(g, wsum, &gtot);
    const u32 eb = block_excl_scan<K7_PICK_THREADS>(e, wsum, &etot);
    if (t < nwg) { a.blk[(size_t)t * 4 + 2] = gb; a.blk[(size_t)t * 4 + 3] = eb; }
    if (t == 0) {
        const u32 need = a.state[K7S_REM];
        const u32 m = gtot + (etot < need ? etot : need);
        a.state[K7S_SEL] = m;
        if (a.n_out) *a.n_out = m;
    }
}

__device__ __forceinline__ void k7_copy_row(sg_edge_out* dst, const sg_edge_out* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* o = reinterpret_cast<uint4*>(dst);
    const uint4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
}

// ordered compaction of the selected rows, in row order (tiles of K7_THREADS rows; a thread's flags are packed gt | eq << 16)
__global__ __launch_bounds__(K7_THREADS) void k7_scatter(SelArgs a) {
    __shared__ u32 wsum[K7_THREADS / 64 + 1];
    const u32 t = threadIdx.x, T = a.state[K7S_PREFIX], need = a.state[K7S_REM];
    const u64 E = k7_rows(a);
    u64 lo, hi; k7_span(E, lo, hi);
    u32 gbase = a.blk[(size_t)blockIdx.x * 4 + 2], ebase = a.blk[(size_t)blockIdx.x * 4 + 3];
    for (u64 i0 = lo; i0 < hi; i0 += K7_THREADS) {                          // (uniform trip count: every thread reaches the barriers)
        const u64 i = i0 + t;
        const u32 key = i < hi ? a.keys[i] : 0u;
        const u32 g = i < hi && key > T, q = i < hi && key == T;
        u32 tot;
        const u32 x = block_excl_scan<K7_THREADS>(g | (q << 16), wsum, &tot);
        const u32 gb = gbase + (x & 0xFFFFu), eb = ebase + (x >> 16);
        if (g || (q && eb < need)) {
            const u64 p = (u64)gb + (eb < need ? eb : need);
            if (a.k) {
                if (p < SG_SELECT_MAX_K) a.pairs[p] = ((u64)(~key) << 32) | (u32)i;
            } else if (p < a.cap) {
                if (a.out) k7_copy_row(a.out + p, a.rows + i);
                if (a.out_idx) a.out_idx[p] = (u32)i;
            }
        }
        gbase += tot & 0xFFFFu; ebase += tot >> 16;
    }
}

// top-k mode, one workgroup: the m = state[SEL] pairs sorted ascending in LDS (bitonic, padded to n = a power of two >= m, pad
// ~0 sorts last), then row j of the output = the row of pair j
__global__ __launch_bounds__(K7_PICK_THREADS) void k7_sort(SelArgs a, u32 n) {
    extern __shared__ u64 sp[];
    const u32 t = threadIdx.x;
    u32 m = a.state[K7S_SEL];
    if (m > n) m = n;
    for (u32 j = t; j < n; j += K7_PICK_THREADS) sp[j] = j < m ? a.pairs[j] : ~0ull;
    __syncthreads();
    for (u32 k = 2; k <= n; k <<= 1) {
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 i = t; i < n; i += K7_PICK_THREADS) {
                const u32 l = i ^ j;
                if (l > i) {
                    const u64 x = sp[i], y = sp[l];
                    if ((x > y) == ((i & k) == 0)) { sp[i] = y; sp[l] = x; }
                }
            }
            __syncthreads();
        }
    }
    const u64 take = m < a.cap ? m : a.cap;
    for (u32 j = t; j < take; j += K7_PICK_THREADS) {
        const u32 i = (u32)sp[j];
        if (a.out) k7_copy_row(a.out + j, a.rows + i);
        if (a.out_idx) a.out_idx[j] = i;
    }
}
