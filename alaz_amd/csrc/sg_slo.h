// sg_slo.h — K24: SLO burn rates per node row and workload row (include/servicegraph.h, "SLO burn rates").  Included after
// sg_quantiles.h and sg_group_nodes.h: it reuses K9's node key (k9_node), K16's group key (k16_gk), K7's passes and k_gather_sel
// unchanged; every kernel here is its own.
//
// The key spaces are small and dense (KNOWN and LABEL ids, and the groups in front of them for the workloads: at most 2^21 keys), so
// the state is indexed by key directly — no sorted merge, no capacity cut, no expiry:
//
//   ring   [L][keys][2 sides][3] u64   the samples (total, err, slow) of the last L windows, slice w mod L the window w's
//   sums   [keys][2 sides][6] u64      T_S, E_S, W_S, T_L, E_L, W_L: the ring's slices summed over the short and the long span
//   obj    [keys] u32                  the objective word (0: the defaults)
//
//   k24_retire   over the keys, in front of the window's samples: the slice that leaves the long span (w mod L, once w >= L) and the
//                one that leaves the short span ((w - S) mod L, once w >= S) are subtracted from their sums, then slice w mod L is
//                zeroed — both slices are read before the store, so S == L (one slice) subtracts it once from each
//   k24_update   over the window's rows, a thread a row: the side counts of the row and the K20 bins above the objective's bin are
//                the sample; it goes to slice w mod L and into both sums, the four burn rates a side follow, and the 18 words are
//                written at the row's position.  K9 and K16 emit one row per ref: a key has one writer, no atomic on the state
//   k24_count    over the keys, for sg_slo_stats_get: the keys with a non-zero T_L
//   k24_keys     the key pass of the two selections: min(short burn, long burn) of a kind and side as K7's key
//
// Integer arithmetic only: r = floor(bad * 2^20 / total) is K10's long division (k10_x_err's steps with the quotient kept a u64:
// exact for every u64 pair, bad <= total so r <= 2^20), burn = r * 10^6 / (budget * 1024) one 64-bit division of a product below 2^40.
#pragma once

#define K24_THREADS 256
#define K24_MAX_WGS 1024
enum { K24C_BURNING = 0, K24C_ACTIVE = 1, K24C_WORDS = 4 };

static_assert(SG_SLO_WORDS == 18 && SG_HIST_BINS == 16, "k24_update writes 2 x 8 + 2 words a row from 16 bins a side");

struct SloArgs {
    GroupNodesArgs g;             // the id spaces: k16_gk for the workloads, g.nd alone (k9_node) for the nodes
    const sg_node_out* nodes;     // the window's node rows / workload rows
    const u64* count;             // their count
    u32 cap;                      // the rows a window can have
    u32 workload;                 // 0: the node space, 1: the workload space
    const u64* hist;              // K20's histograms of the slot: [rows][2][16], side 0 = out, 1 = in
    u32 keys, S, L;
    u64 w;                        // windows closed before this one
    u32 bin, lat_budget, err_budget, min_burn;   // the defaults (budgets in ppm) and the threshold
    u64 min_requests;
    u64* ring; u64* sums; const u32* obj; u64* ctl;
    u64* out;                     // [cap][SG_SLO_WORDS] this window's rows
};

// the key of a ref, SG_NONE for an untracked one (OBIP, or beyond the id spaces: no window has such a row)
__device__ __forceinline__ u32 k24_key(const SloArgs& a, u32 ref) {
    if (SG_REF_TYPE(ref) == SG_REF_OBIP) return SG_NONE;
    const u32 k = a.workload ? k16_gk(a.g, ref) : k9_node(a.g.nd, ref);
    return k < a.keys ? k : SG_NONE;
}
__device__ __forceinline__ u32 k24_budget(u32 code) {
    const u32 e = code >> 10, p = e == 0 ? 1u : e == 1 ? 10u : e == 2 ? 100u : 1000u, b = (code & 1023u) * p;
    return b ? b : 1u;                                               // (sg_slo_assign admits no code of budget 0)
}
__device__ __forceinline__ u32 k24_burn(u64 bad, u64 total, u32 budget) {
    if (!total) return 0u;
    if (bad > total) bad = total;
    u64 r = bad / total, rem = bad % total;                           // floor(bad * 2^20 / total) <= 2^20: the integer part shifted,
    for (int b = 0; b < 20; b++) {                                    // the twenty fraction bits one at a time, the carry bit kept
        const u64 hi = rem >> 63;
        rem <<= 1;
        r <<= 1;
        if (hi || rem >= total) { rem -= total; r |= 1u; }
    }
    return (u32)(r * 1000000ull / ((u64)budget * 1024ull));
}

__global__ __launch_bounds__(K24_THREADS) void k24_retire(SloArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[K24C_BURNING] = 0;
    const bool longs = a.w >= a.L, shorts = a.w >= a.S;
    const u64 sl = a.w % a.L, ss = shorts ? (a.w - a.S) % a.L : sl;
    for (u64 k = (u64)blockIdx.x * K24_THREADS + threadIdx.x; k < a.keys; k += (u64)gridDim.x * K24_THREADS) {
        u64* cur = a.ring + (sl * a.keys + k) * 6;
        const u64* old = a.ring + (ss * a.keys + k) * 6;
        u64 lo[6], sh[6], any = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) { lo[i] = cur[i]; sh[i] = old[i]; any |= lo[i] | sh[i]; }
        if (!any) continue;                                          // (a zero slice stays zero, nothing leaves a sum)
        u64* s = a.sums + k * 12;
#pragma unroll
        for (int side = 0; side < 2; side++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (shorts) s[side * 6 + j] -= sh[side * 3 + j];
                if (longs) s[side * 6 + 3 + j] -= lo[side * 3 + j];
            }
#pragma unroll
        for (int i = 0; i < 6; i++) cur[i] = 0;
    }
}

__global__ __launch_bounds__(K24_THREADS) void k24_update(SloArgs a) {
    const u64 N = sg_nodes_of(a.count, a.cap);
    const u64 sl = a.w % a.L;
    const u64 spans = (a.w + 1 < a.S ? a.w + 1 : (u64)a.S) | (a.w + 1 < a.L ? a.w + 1 : (u64)a.L) << 32;
    for (u64 v = (u64)blockIdx.x * K24_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K24_THREADS) {
        const u64* r = reinterpret_cast<const u64*>(a.nodes + v);     // words: 0 / 1 counts, 2 / 3 errors (out / in); ref: byte 96
        u64* o = a.out + v * SG_SLO_WORDS;
        const u32 key = k24_key(a, reinterpret_cast<const u32*>(r)[24]);
        if (key == SG_NONE) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[i] = 0;
            o[16] = SG_SLO_UNTRACKED; o[17] = 0;
            continue;
        }
        const u32 word = a.obj[key];
        const u32 bin = word ? word >> 28 : a.bin;
        const u32 lat_budget = word ? k24_budget(word >> 12 & 0xFFFu) : a.lat_budget, err_budget = word ? k24_budget(word & 0xFFFu) : a.err_budget;
        u64* ring = a.ring + (sl * a.keys + key) * 6;
        u64* sums = a.sums + (u64)key * 12;
        u32 flags = 0, burning = 0;
#pragma unroll
        for (int side = 0; side < 2; side++) {                       // 0 = in, 1 = out; K20's tables hold a side as 1 - side
            const u64 total = r[1 - side];
            u64 err = 0, slow = 0;
            if (total) {
                err = r[3 - side];
                const u64* h = a.hist + (v * 2 + (1 - side)) * SG_HIST_BINS;
                for (u32 b = bin + 1; b < SG_HIST_BINS; b++) slow += h[b];
            }
            ring[side * 3] = total; ring[side * 3 + 1] = err; ring[side * 3 + 2] = slow;
            u64* s = sums + side * 6;
            const u64 ts = s[0] + total, es = s[1] + err, ws = s[2] + slow, tl = s[3] + total, el = s[4] + err, wl = s[5] + slow;
            s[0] = ts; s[1] = es; s[2] = ws; s[3] = tl; s[4] = el; s[5] = wl;
            const u32 bes = k24_burn(es, ts, err_budget), bel = k24_burn(el, tl, err_budget);
            const u32 bws = k24_burn(ws, ts, lat_budget), bwl = k24_burn(wl, tl, lat_budget);
            u64* q = o + side * 8;
            q[0] = ts; q[1] = es; q[2] = ws; q[3] = tl; q[4] = el; q[5] = wl;
            q[6] = (u64)bes | (u64)bel << 32; q[7] = (u64)bws | (u64)bwl << 32;
            const bool gate = tl >= a.min_requests;
            const u32 f = (gate && bes >= a.min_burn && bel >= a.min_burn ? SG_SLO_ERR_BURNING_IN : 0u) |
                          (gate && bws >= a.min_burn && bwl >= a.min_burn ? SG_SLO_SLOW_BURNING_IN : 0u);
            flags |= f << (2 * side);
            burning += f ? 1u : 0u;
        }
        o[16] = (u64)flags | (u64)word << 32; o[17] = spans;
        if (burning) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + K24C_BURNING), (unsigned long long)burning);
    }
}

// the keys with traffic in the long span, added to ctl[K24C_ACTIVE] (the host zeroes it in front)
__global__ __launch_bounds__(K24_THREADS) void k24_count(const u64* sums, u32 keys, u64* ctl) {
    u32 c = 0;
    for (u64 k = (u64)blockIdx.x * K24_THREADS + threadIdx.x; k < keys; k += (u64)gridDim.x * K24_THREADS) c += (sums[k * 12 + 3] | sums[k * 12 + 9]) != 0ull;
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(reinterpret_cast<unsigned long long*>(ctl + K24C_ACTIVE), (unsigned long long)c);
}

// ---- selection by a burn rate ---------------------------------------------------------------------------------------------------
// k7_keys over SLO rows alone (k10_keys' shape): the value of row i is min(short, long) of word 8 * side + 6 + kind, 0 when the
// row is untracked or its T_L (word 8 * side + 3) is below min_requests; a value >= min_value is a candidate with key
// value | 2^31 (a burn is below 2^30: larger value, larger key, every candidate key > 0).  The entity rows are not read.  Workgroup 0
// resets K7's state and copies the row count to ctr[C_N_EDGES], where K7's later passes read it (a.ctr = ctr).  i < E <=
// a.max_edges, the rows a slot's SLO rows hold.
__global__ __launch_bounds__(K7_THREADS) void k24_keys(SelArgs a, const u64* count, const u64* rows, u32 side, u32 kind, u32 min_value, u64 min_requests,
                                                       u64* ctr) {
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
        const u64* r = rows + i * SG_SLO_WORDS;
        const u64 b = r[8 * side + 6 + kind];
        const u32 bs = (u32)b, bl = (u32)(b >> 32);
        u32 v = bs < bl ? bs : bl;
        if ((r[16] & SG_SLO_UNTRACKED) || r[8 * side + 3] < min_requests) v = 0;
        const u32 key = v >= min_value ? v | 0x80000000u : 0u;
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}
