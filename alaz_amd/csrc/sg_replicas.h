// sg_replicas.h — K25: replica outliers, each pod against the other pods of its workload (include/servicegraph.h, "replica
// outliers").  Included after sg_slo.h: it reuses K9's node key (k9_node), K16's group key (k16_gk), k20_pos_groups (over a position
// table of its own), K7's passes and k_gather_sel unchanged; every kernel here is its own.
//
// Work is in ROW-INDEX space, in K20's shape.  The stage keeps nothing across windows:
//
//   k20_pos_groups  (sg_quantiles.h, unchanged) per workload row w: pos[k16_gk(ref_w)] = w.  Only the window's keys are written
//   k25_member   per node row v: the workload row it is a member of -> tgt[v], SG_NONE for a non-member.  A member's ref is KNOWN,
//                its kind is SG_NODE_POD, the map gives it a group g, and the workload row at pos[g] carries the ref GROUP | g (a
//                position a window before left in the table fails that test)
//   k25_fold     ONE body, two policies.  Workgroup (range, slice): range_rows workload rows x `words` u64 in LDS (64 KiB at most:
//                two workgroups a CU).  The targets do not ascend with the node rows (pods are ordered by id, workloads by group key):
//                every range scans its slice of the 4-byte targets and loads only the rows whose target is in range; what a row adds
//                goes in with LDS integer atomics, and the LDS goes to the (range, slice) partial.  A workload with many replicas is
//                spread over the slices and the lanes; device memory sees no atomic at all.  Integer adds and one integer min only:
//                the partials' fold does not depend on the split
//                  K25Sums     a member's node row (and, with tails, its two K20 node histograms): R, C, E, T and H[16] a side
//                  K25Verdict  a member's pod row: judged sides, outlier sides, the smallest node row among the outlier sides
//   k25_reduce   the slices' partials of the member sums added up into one table [workload rows][words]
//   k25_rows     per node row: the leave-one-out values, the flags, the pod row
//   k25_groups   per workload row: R from the sums' table, the slices' partials of the verdicts folded, the workload row
//   k25_keys     the key pass of sg_window_replicas_top
//
// Every kernel here is a TEMPLATE (the plain ones over a dummy `int V = 0`, launched as k25_x<0>): the compiler emits a translation
// unit's plain kernels first and its template instantiations behind them, in the order of their first use, so as plain functions these
// kernels sat in front of K1 - K5's instantiations in the code object and moved every one of them; with the stage off the benchmark
// then ran below the parent's in every alternated pair (profiles/replica_ab.txt).  As templates they come behind the hot kernels.
//
// Integer arithmetic only: x_err is K10's sample by long division (k24_burn's steps), the ratios are 64-bit divisions of products
// below 2^64 (mean <= 2^52, c <= 2^53).
#pragma once

#define K25_THREADS 256
#define K25_MAX_WGS 1024
#define K25_SIDE_WORDS 4          // R, C, E, T; with tails the 16 bins behind them
#define K25_VERDICT_WORDS 6       // judged, outliers, first outlier: the in side, then the out side

static_assert(SG_REPLICA_WORDS == 12 && SG_REPLICA_GROUP_WORDS == 8 && SG_HIST_BINS == 16 && SG_REPL_JUDGED_OUT == SG_REPL_JUDGED_IN << 4,
              "k25_rows writes 2 + 2 x 5 words a pod row, a side's flags four bits apart");

struct ReplicaArgs {
    GroupNodesArgs g;             // the id spaces and the group keys (k16_gk)
    const u32* map;               // [max_known] K14's group map, as the window was contracted under it
    const uint8_t* kind;          // [max_known] SG_NODE_POD / SG_NODE_SERVICE
    const sg_node_out* nodes; const u64* ncount; u32 ncap;   // the window's node rows
    const sg_node_out* wrows; const u64* wcount; u32 nc;     // the window's workload rows
    const u64* hist;              // K20's node histograms of the slot: [rows][2][16], side 0 = out, 1 = in (tails only)
    u32 tails, words;             // words: u64 words a workload row of the member sums
    u32 range_rows, slices;
    u32 min_replicas, min_err, min_lat, permille, min_tail;
    u64 min_requests;
    u32* pos; u32* tgt;
    u64* part; u64* vpart; u64* wsum;
    u32* pods;                    // [ncap][SG_REPLICA_WORDS] this window's pod rows
    u32* groups;                  // [nc][SG_REPLICA_GROUP_WORDS] this window's workload rows
};

template <int V = 0>
__global__ __launch_bounds__(K25_THREADS) void k25_member(ReplicaArgs a) {
    const u64 N = sg_nodes_of(a.ncount, a.ncap), NW = sg_nodes_of(a.wcount, a.nc);
    for (u64 v = (u64)blockIdx.x * K25_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K25_THREADS) {
        const u32 ref = a.nodes[v].ref, id = SG_REF_VALUE(ref);
        u32 w = SG_NONE;
        if (SG_REF_TYPE(ref) == SG_REF_KNOWN && id < a.g.nd.mk && a.kind[id] == SG_NODE_POD) {
            const u32 g = a.map[id];
            if (g != SG_NO_GROUP && g < a.g.max_groups && g < a.g.gk) {
                const u32 p = a.pos[g];
                if (p < NW && a.wrows[p].ref == SG_MAKE_REF(SG_REF_GROUP, g)) w = p;
            }
        }
        a.tgt[v] = w;
    }
}

// the member sums: word side * (4 + bins) + j of a workload row, side 0 = in; a node row holds a side's words at 1 - side (the out
// side first), as K20's histograms do
struct K25Sums {
    static __device__ __forceinline__ u32 words(const ReplicaArgs& a) { return a.words; }
    static __device__ __forceinline__ u64 init(u32) { return 0ull; }
    static __device__ __forceinline__ u64* part(const ReplicaArgs& a) { return a.part; }
    static __device__ __forceinline__ void add(const ReplicaArgs& a, u64* acc, u64 v) {
        const u64* r = reinterpret_cast<const u64*>(a.nodes + v);     // words: 0 / 1 counts, 2 / 3 errors, 4 / 5 sums (out / in)
        const u32 sw = a.words >> 1;
        // every load of the member is issued in front of the first atomic: the six row words and, with tails, its two histograms as
        // sixteen 16-byte loads (a bin at a time behind an atomic each was one memory latency a bin: 57 us a launch at config 3)
        u64 w[6];
#pragma unroll
        for (u32 i = 0; i < 6; i++) w[i] = r[i];
        ulonglong2 h[2][SG_HIST_BINS / 2] = {};
        if (a.tails) {
            const ulonglong2* hp = reinterpret_cast<const ulonglong2*>(a.hist + v * 2 * SG_HIST_BINS);   // [out][16], [in][16]: 128-byte entries
#pragma unroll
            for (u32 i = 0; i < SG_HIST_BINS; i++) h[i / (SG_HIST_BINS / 2)][i % (SG_HIST_BINS / 2)] = hp[i];
        }
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            u64* s = acc + side * sw;
            const u64 c = w[1 - side], e = w[3 - side], t = w[5 - side];
            if (c) { atomicAdd(&s[0], 1ull); atomicAdd(&s[1], c); }
            if (e) atomicAdd(&s[2], e);
            if (t) atomicAdd(&s[3], t);
            if (a.tails) {
#pragma unroll
                for (u32 i = 0; i < SG_HIST_BINS / 2; i++) {
                    const ulonglong2 x = h[1 - side][i];
                    if (x.x) atomicAdd(&s[K25_SIDE_WORDS + 2 * i], x.x);
                    if (x.y) atomicAdd(&s[K25_SIDE_WORDS + 2 * i + 1], x.y);
                }
            }
        }
    }
};
// the verdicts: per side judged members, outlier members and the smallest node row among the outlier members
struct K25Verdict {
    static __device__ __forceinline__ u32 words(const ReplicaArgs&) { return K25_VERDICT_WORDS; }
    static __device__ __forceinline__ u64 init(u32 j) { return j % 3 == 2 ? ~0ull : 0ull; }
    static __device__ __forceinline__ u64* part(const ReplicaArgs& a) { return a.vpart; }
    static __device__ __forceinline__ void add(const ReplicaArgs& a, u64* acc, u64 v) {
        const u32 flags = a.pods[v * SG_REPLICA_WORDS + 1];
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 f = flags >> (4 * side);
            if (f & SG_REPL_JUDGED_IN) atomicAdd(&acc[side * 3], 1ull);
            if (f & (SG_REPL_ERR_IN | SG_REPL_LAT_IN | SG_REPL_TAIL_IN)) { atomicAdd(&acc[side * 3 + 1], 1ull); atomicMin(&acc[side * 3 + 2], v); }
        }
    }
};

template <class P>
__global__ __launch_bounds__(K25_THREADS) void k25_fold(ReplicaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* acc = reinterpret_cast<u64*>(smem);
    const u32 S = a.slices, rg = blockIdx.x / S, sl = blockIdx.x % S, t = threadIdx.x, W = P::words(a);
    const u64 NW = sg_nodes_of(a.wcount, a.nc), first = (u64)rg * a.range_rows;
    if (first >= NW) return;                                         // (uniform; nothing reads a partial of such a range)
    const u32 n0 = (u32)first, nr = NW - first < a.range_rows ? (u32)(NW - first) : a.range_rows;
    for (u32 i = t; i < nr * W; i += K25_THREADS) acc[i] = P::init(i % W);
    const u64 N = sg_nodes_of(a.ncount, a.ncap), per = (N + S - 1) / S;
    const u64 p0 = (u64)sl * per < N ? (u64)sl * per : N, p1 = p0 + per < N ? p0 + per : N;
    __syncthreads();
    for (u64 v = p0 + t; v < p1; v += K25_THREADS) {
        const u32 to = a.tgt[v] - n0;                                // (SG_NONE - n0 is beyond every range)
        if (to < nr) P::add(a, acc + (size_t)to * W, v);
    }
    __syncthreads();
    u64* out = P::part(a) + ((size_t)rg * S + sl) * a.range_rows * W;
    for (u32 i = t; i < nr * W; i += K25_THREADS) out[i] = acc[i];
}

template <int V = 0>
__global__ __launch_bounds__(K25_THREADS) void k25_reduce(ReplicaArgs a) {
    const u64 NW = sg_nodes_of(a.wcount, a.nc), W = a.words, S = a.slices, RR = a.range_rows;
    for (u64 x = (u64)blockIdx.x * K25_THREADS + threadIdx.x; x < NW * W; x += (u64)gridDim.x * K25_THREADS) {
        const u64 w = x / W, j = x - w * W, rg = w / RR, i = w - rg * RR;
        const u64* p = a.part + ((rg * S) * RR + i) * W + j;
        u64 s = 0;
        for (u64 sl = 0; sl < S; sl++) s += p[sl * RR * W];
        a.wsum[x] = s;
    }
}

// floor(min(e, c) * 2^20 / c), c > 0: the integer part shifted, the twenty fraction bits one at a time, the carry bit kept
__device__ __forceinline__ u32 k25_x_err(u64 e, u64 c) {
    if (e > c) e = c;
    u64 r = e / c, rem = e % c;
    for (int b = 0; b < 20; b++) {
        const u64 hi = rem >> 63;
        rem <<= 1;
        r <<= 1;
        if (hi || rem >= c) { rem -= c; r |= 1u; }
    }
    return (u32)r;
}
__device__ __forceinline__ u64 k25_mean(u64 s, u64 c) { const u64 m = s / c; return m < (1ull << 52) ? m : (1ull << 52); }
__device__ __forceinline__ u32 k25_clamp32(u64 x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)x; }
// the first bin whose cumulative count reaches K20's rank (k20_quantile's), 15 when none does, 0 without requests
__device__ __forceinline__ u32 k25_qbin(const u64* h, u32 qm) {
    u64 total = 0;
#pragma unroll
    for (u32 b = 0; b < SG_HIST_BINS; b++) total += h[b];
    if (!total) return 0u;
    u64 rank = (total / 1000ull) * qm + ((total % 1000ull) * qm + 999ull) / 1000ull;
    rank = rank ? rank : 1ull;
    u64 cum = 0;
    u32 bq = SG_HIST_BINS - 1; bool found = false;
#pragma unroll
    for (u32 b = 0; b < SG_HIST_BINS; b++) { cum += h[b]; if (!found && cum >= rank) { bq = b; found = true; } }
    return bq;
}

template <int V = 0>
__global__ __launch_bounds__(K25_THREADS) void k25_rows(ReplicaArgs a) {
    const u64 N = sg_nodes_of(a.ncount, a.ncap);
    const u32 sw = a.words >> 1;
    for (u64 v = (u64)blockIdx.x * K25_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K25_THREADS) {
        u32* o = a.pods + v * SG_REPLICA_WORDS;
        const u32 w = a.tgt[v];
        if (w == SG_NONE) {
            o[0] = SG_NONE;
#pragma unroll
            for (int i = 1; i < (int)SG_REPLICA_WORDS; i++) o[i] = 0;
            continue;
        }
        const u64* r = reinterpret_cast<const u64*>(a.nodes + v);
        u32 flags = SG_REPL_MEMBER;
        o[0] = w;
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u64* s = a.wsum + (u64)w * a.words + side * sw;
            const u64 R = s[0], C = s[1], E = s[2], T = s[3];
            const u64 c = r[1 - side], e = r[3 - side], t = r[5 - side];
            u32 excess = 0, ratio = 0, share = 0, tail = 0, f = 0;
            if (c >= a.min_requests && C - c >= a.min_requests && R >= a.min_replicas) {
                f = SG_REPL_JUDGED_IN;
                const int ex = (int)k25_x_err(e, c) - (int)k25_x_err(E - e, C - c);
                excess = (u32)ex;
                const u64 mp = k25_mean(T - t, C - c);
                ratio = k25_clamp32(k25_mean(t, c) * 1024ull / (mp ? mp : 1ull));
                const u64 fair = C / R;
                share = k25_clamp32((c < (1ull << 53) ? c : (1ull << 53)) * 1024ull / (fair ? fair : 1ull));
                if (ex >= (int)a.min_err) f |= SG_REPL_ERR_IN;
                if (ratio >= a.min_lat) f |= SG_REPL_LAT_IN;
                if (a.tails) {
                    const u64* h = a.hist + (v * 2 + (1 - side)) * SG_HIST_BINS;
                    u64 hp[SG_HIST_BINS], hq[SG_HIST_BINS];
#pragma unroll
                    for (u32 b = 0; b < SG_HIST_BINS; b++) { hp[b] = h[b]; hq[b] = s[K25_SIDE_WORDS + b] - hp[b]; }
                    const u32 tp = k25_qbin(hp, a.permille), tq = k25_qbin(hq, a.permille);
                    tail = tp | tq << 8;
                    if ((int)tp - (int)tq >= (int)a.min_tail) f |= SG_REPL_TAIL_IN;
                }
            }
            u32* q = o + 2 + side * 5;
            q[0] = excess; q[1] = ratio; q[2] = share; q[3] = tail; q[4] = (u32)R;
            flags |= f << (4 * side);
        }
        o[1] = flags;
    }
}

template <int V = 0>
__global__ __launch_bounds__(K25_THREADS) void k25_groups(ReplicaArgs a) {
    const u64 NW = sg_nodes_of(a.wcount, a.nc), S = a.slices, RR = a.range_rows;
    const u32 sw = a.words >> 1;
    for (u64 w = (u64)blockIdx.x * K25_THREADS + threadIdx.x; w < NW; w += (u64)gridDim.x * K25_THREADS) {
        const u64 rg = w / RR, i = w - rg * RR;
        const u64* p = a.vpart + ((rg * S) * RR + i) * K25_VERDICT_WORDS;
        u64 x[K25_VERDICT_WORDS] = {0, 0, ~0ull, 0, 0, ~0ull};
        for (u64 sl = 0; sl < S; sl++) {
            const u64* q = p + sl * RR * K25_VERDICT_WORDS;
#pragma unroll
            for (u32 side = 0; side < 2; side++) {
                x[side * 3] += q[side * 3]; x[side * 3 + 1] += q[side * 3 + 1];
                x[side * 3 + 2] = q[side * 3 + 2] < x[side * 3 + 2] ? q[side * 3 + 2] : x[side * 3 + 2];
            }
        }
        u32* o = a.groups + w * SG_REPLICA_GROUP_WORDS;
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            o[side * 4] = (u32)a.wsum[w * a.words + side * sw];
            o[side * 4 + 1] = (u32)x[side * 3]; o[side * 4 + 2] = (u32)x[side * 3 + 1]; o[side * 4 + 3] = (u32)x[side * 3 + 2];
        }
    }
}

// ---- selection over the pod rows ----------------------------------------------------------------------------------------------------
// k7_keys over pod rows alone (k24_keys' shape): the value of row i is max(err_excess_q20, 0), lat_ratio_q10, max(tail_excess, 0) or
// share_q10 (kind 0 .. 3) of side `side` when that side is judged, else 0; a value >= min_value and > 0 is a candidate and its own
// key (a u32: larger value, larger key).  The node rows are not read.  Workgroup 0 resets K7's state and copies the row count to
// ctr[C_N_EDGES], where K7's later passes read it (a.ctr = ctr).  i < E <= a.max_edges, the rows a slot's pod rows hold.
template <int V = 0>
__global__ __launch_bounds__(K7_THREADS) void k25_keys(SelArgs a, const u64* count, const u32* pods, u32 side, u32 kind, u32 min_value, u64* ctr) {
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
        const u32* r = pods + i * SG_REPLICA_WORDS;
        const u32* q = r + 2 + side * 5;
        u32 v = 0;
        if (r[1] & (SG_REPL_JUDGED_IN << (4 * side))) {
            if (kind == 0) v = (int)q[0] > 0 ? q[0] : 0u;
            else if (kind == 1) v = q[1];
            else if (kind == 2) { const int d = (int)(q[3] & 255u) - (int)(q[3] >> 8 & 255u); v = d > 0 ? (u32)d : 0u; }
            else v = q[2];
        }
        const u32 key = v >= min_value ? v : 0u;
        a.keys[i] = key;
        if (key && a.k) atomicAdd(&h[key >> 24], 1u);
    }
    __syncthreads();
    a.hist[(size_t)blockIdx.x * 256 + t] = h[t];
}
