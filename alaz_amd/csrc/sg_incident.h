// sg_incident.h — K12: each window's anomalous rows grouped into incidents on the device (include/servicegraph.h, "incidents"),
// and the passes K12 shares with K18, the workload incidents (sg_group_incident.h).
// Included after sg_rank.h: it reuses K9's node key (k9_node), K9's node rows and k9_scan unchanged, and adds kernels of its own.
//
// An incident is a connected component of the window's graph restricted to its red rows (value >= min_value).  Work is in K9's
// node-key space (k9_node(ref) < ncap); keys are monotone in node order, so the smallest key of a component belongs to its
// first_node.  Only the keys of the window's node rows are ever read or written, so nothing is zeroed between windows.  Every field
// of an incident is an integer sum, an integer max or the max of a 64-bit key (order-preserving bits << 32 | ~index), so the result
// has one value whatever order the workgroups and lanes run in.  Eight plain launches on the window's stream; no workgroup ever
// waits for another: the only loops over shared state are CAS retries (another hook succeeded) and root walks (parent[x] < x).
//
//   k12_init    per node row: parent[key] = key, flag[key] = 0
//   k12_hook    per row: red?  Then flag both endpoints and unite them: lock-free union-find with min-hooking — find both roots
//               (path halving), hook the larger root under the smaller with a CAS on the larger root's word, retry from the new
//               roots when it fails.  parent[x] <= x always, so a component's final root is its smallest key.  parent[] is shared
//               by every workgroup of this launch and the CUs' L1s are not coherent inside one: every access to it here is an
//               agent-scope relaxed atomic (load, store or CAS).
//   k12_label   per node row (a later launch: plain loads): lab[key] = root(key); heads (flagged and lab == key) counted per workgroup
//   k9_scan     (1 workgroup, K9's kernel) exclusive scan of the counts; the incident count of the window
//   k12_number  per node row: a head's incident number is its exclusive rank: num[key]; the incident's accumulators start here
//   k12_nodes   per node row: its incident (the window's sg_window_node_incident row, and kinc[key] for the rows' pass); nodes,
//               the top node's key, rank_sum and the largest rank folded per incident
//   k12_rows    per red row, under the incident of its source: edges, count, err, sum_ns, score_q32, the worst row's key; beside
//               it per node row: culprit_node = the smallest node row whose rank is the incident's largest
//   k12_finish  per incident: value_max / worst_row and top_node out of their keys
//
// The two folding passes never issue a device atomic per row: a wave whose active lanes all name one incident (rows are sorted by
// source: the common case) reduces them in registers first, every contribution then goes to an LDS table keyed by incident (LDS
// atomics), and a workgroup touches device memory once per field and distinct incident it met, skipping fields with nothing to
// add.  Only an incident that finds no table slot (K12_PROBES probes of K12_SLOTS) is added to device memory directly.
//
// All but the first two passes are one body each (k12_label_t, k12_number_t, k12_nodes_t, k12_rows_t, k12_finish_t) over a space
// policy: K12Space here, K18Space in sg_group_incident.h.  The policy answers what differs between the two spaces — the row counts,
// the array index of a node row, where k9_scan's words live, what the node fold keeps for the rows pass and how the rows pass
// loads one row — and the __global__ kernels of both files are wrappers that name the space.  k12_init / k12_hook and k18_init /
// k18_hook stay per space: they read different row formats and write different arrays (pos in k18_init, esrc in k18_hook), and
// share k12_unite.
#pragma once

#define K12_THREADS 256           // every pass of K12 and K18
#define K12_SLOTS 512             // LDS table of the folding passes: incidents per workgroup before it falls back to device atomics
#define K12_PROBES 8
#define K12_MAX_WGS 1024          // node workgroups at most (k9_scan scans one count per thread)
#define K12_EMPTY 0xFFFFFFFFu

static_assert(sizeof(sg_incident_out) == 72 && offsetof(sg_incident_out, first_node) == 40 && offsetof(sg_incident_out, value_max) == 64 &&
              sizeof(sg_incident_params) == 16, "sg_incident_out / sg_incident_params layout");
static_assert(K12_MAX_WGS == K9_MAX_WGS && K12_MAX_WGS <= K9_SCAN_THREADS, "k9_scan scans the head counts of K12 and K18");

// what the key pass of a max field keeps per incident until k12_finish (scratch shared by the window slots)
struct K12Keys { u64 worst, top, rmax; };

struct IncArgs {
    NodesArgs nd;                 // K9's part: rows, ctr, max_edges, mk, ml, mob, ncap (k9_node, k9_rows_of); blk, count: k9_scan's
    const sg_node_out* nodes;     // the window's node rows
    const u64* ncount;            // their count
    const sg_edge_trend* trend;   // the window's trend rows (a trend key), else unused
    const sg_node_rank* rank;     // the window's rank rows, NULL with the ranking off
    u32 by; float min_value;
    u32 node_per;                 // node rows per workgroup of k12_label / k12_number (a multiple of K12_THREADS)
    u32* parent; u32* flag; u32* lab; u32* num; u32* kinc;   // [ncap] by node key
    K12Keys* keys;                // [ncap] by incident
    sg_incident_out* out;         // [ncap] this window's incidents (nd.count: their count)
    u32* node_inc;                // [ncap] this window's incident per node row
};

// the row's value, and whether it is red
__device__ __forceinline__ bool k12_red(const IncArgs& a, u64 j, u32 s, u32 d, float score, float& value) {
    value = a.by == SG_SEL_SCORE ? score : a.by == SG_SEL_LAT_DEV ? a.trend[j].lat_dev : a.trend[j].err_dev;
    return s != SG_NONE && d != SG_NONE && value >= a.min_value;
}

__device__ __forceinline__ u32 k12_ld(u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the root of x, halving the path on the way (a node that is not a root never becomes one again, and every value stored is an
// ancestor: concurrent halvings and hooks cannot break the tree)
__device__ __forceinline__ u32 k12_find(u32* parent, u32 x) {
    for (;;) {
        const u32 p = k12_ld(parent + x);
        if (p == x) return x;
        const u32 gp = k12_ld(parent + p);
        if (gp == p) return p;
        __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
}
__device__ __forceinline__ void k12_unite(u32* parent, u32 x, u32 y) {
    u32 a = k12_find(parent, x), b = k12_find(parent, y);
    while (a != b) {
        const u32 hi = a > b ? a : b, lo = a > b ? b : a;
        u32 expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = k12_find(parent, hi); b = k12_find(parent, lo);         // (hi was hooked by another row meanwhile: from the new roots)
    }
}

__global__ __launch_bounds__(K12_THREADS) void k12_init(IncArgs a) {
    const u64 N = sg_nodes_of(a.ncount, a.nd.ncap);
    for (u64 v = (u64)blockIdx.x * K12_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K12_THREADS) {
        const u32 k = k9_node(a.nd, a.nodes[v].ref);
        if (k == SG_NONE) continue;                                   // (cannot be: K9 made the row from such a key)
        a.parent[k] = k; a.flag[k] = 0;
    }
}

__global__ __launch_bounds__(K12_THREADS) void k12_hook(IncArgs a) {
    const u64 E = k9_rows_of(a.nd);
    for (u64 j = (u64)blockIdx.x * K12_THREADS + threadIdx.x; j < E; j += (u64)gridDim.x * K12_THREADS) {
        const u64* r = reinterpret_cast<const u64*>(a.nd.rows + j);  // word 3: from | to << 32; word 5 low: the score (sg_k5.h)
        const u64 ft = r[3];
        const u32 s = k9_node(a.nd, (u32)ft), d = k9_node(a.nd, (u32)(ft >> 32));
        float value;
        if (!k12_red(a, j, s, d, __uint_as_float((u32)r[5]), value)) continue;
        a.flag[s] = 1; a.flag[d] = 1;                                 // (every writer stores 1; read by the next launch)
        if (s != d) k12_unite(a.parent, s, d);
    }
}

// K12's space: parent, flag, lab and num are indexed by node key, and kinc[key] hands a node's incident to the rows pass, which
// knows its rows' endpoints by key only
struct K12Space {
    typedef IncArgs Args;
    static __device__ __forceinline__ u64 nodes(const IncArgs& a) { return sg_nodes_of(a.ncount, a.nd.ncap); }
    static __device__ __forceinline__ u64 rows(const IncArgs& a) { return k9_rows_of(a.nd); }
    // the array index of node row v; false: it has none (cannot be: K9 made the row from such a key)
    static __device__ __forceinline__ bool index(const IncArgs& a, u64 v, u32& k) { k = k9_node(a.nd, a.nodes[v].ref); return k != SG_NONE; }
    static __device__ __forceinline__ const NodesArgs& scan(const IncArgs& a) { return a.nd; }
    static __device__ __forceinline__ void keep(const IncArgs& a, u32 k, u32 i) { a.kinc[k] = i; }
    // row j's incident, SG_NO_INCIDENT unless it is red, and what it adds: count, err, sum_ns, score_q32 and its worst-row key
    static __device__ __forceinline__ u32 row(const IncArgs& a, u64 j, u64& xc, u64& xe, u64& xs, u64& xq, u64& xw) {
        const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.nd.rows + j);   // words 0..5 (sg_k5.h; k9_load)
        const ulonglong2 w23 = r[1], w45 = r[2];
        const u32 s = k9_node(a.nd, (u32)w23.y), d = k9_node(a.nd, (u32)(w23.y >> 32));
        const float score = __uint_as_float((u32)w45.y);
        float value;
        if (!k12_red(a, j, s, d, score, value)) return SG_NO_INCIDENT;
        xc = (u32)w45.x; xe = (u32)(w45.x >> 32); xs = r[0].x; xq = k9_q32(score); xw = k9_worst_key(value, j);
        return a.kinc[s];
    }
};

// the workgroup's node rows [v0, v1) in rounds of K12_THREADS
__device__ __forceinline__ void k12_node_span(u32 node_per, u64 N, u64& v0, u64& v1) {
    v0 = (u64)blockIdx.x * node_per; v1 = v0 + node_per;
    if (v0 > N) v0 = N;
    if (v1 > N) v1 = N;
}

template <class S>
__device__ __forceinline__ void k12_label_t(const typename S::Args& a) {
    __shared__ u32 ws[K12_THREADS / 64];
    const u32 t = threadIdx.x;
    u64 v0, v1; k12_node_span(a.node_per, S::nodes(a), v0, v1);
    u32 c = 0;
    for (u64 v = v0 + t; v < v1; v += K12_THREADS) {
        u32 k;
        if (!S::index(a, v, k)) continue;
        u32 x = k;
        for (u32 p = a.parent[x]; p != x; p = a.parent[x]) x = p;    // (strictly descending, p < x: it ends at a root)
        a.lab[k] = x;
        c += (x == k && a.flag[k]) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if ((t & 63) == 0) ws[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        u32 s = 0;
        for (int w = 0; w < K12_THREADS / 64; w++) s += ws[w];
        S::scan(a).blk[blockIdx.x] = s;
    }
}

template <class S>
__device__ __forceinline__ void k12_number_t(const typename S::Args& a) {
    __shared__ u32 wsum[K12_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    u64 v0, v1; k12_node_span(a.node_per, S::nodes(a), v0, v1);
    u32 base = S::scan(a).blk[K12_MAX_WGS + blockIdx.x];
    for (u64 vb = v0; vb < v1; vb += K12_THREADS) {                 // (uniform: every thread takes every round)
        const u64 v = vb + t;
        u32 k = SG_NONE;
        bool head = false;
        if (v < v1 && S::index(a, v, k)) head = a.lab[k] == k && a.flag[k];
        u32 tot;
        const u32 x = block_excl_scan<K12_THREADS>(head ? 1u : 0u, wsum, &tot);
        if (head) {
            const u32 i = base + x;
            a.num[k] = i;
            sg_incident_out o{};
            o.first_node = (u32)v; o.worst_row = SG_NO_INCIDENT; o.top_node = SG_NO_INCIDENT; o.culprit_node = SG_NO_INCIDENT;
            a.out[i] = o;
            K12Keys z; z.worst = z.top = z.rmax = 0;
            a.keys[i] = z;
        }
        base += tot;
    }
}

// the LDS table's slot of incident i, or K12_EMPTY when K12_PROBES probes find none
__device__ __forceinline__ u32 k12_slot(u32* key, u32 i) {
    u32 h = (i * 2654435761u) >> 23;                                  // (K12_SLOTS = 2^9)
#pragma unroll 1
    for (int p = 0; p < K12_PROBES; p++) {
        const u32 old = atomicCAS(&key[h], K12_EMPTY, i);
        if (old == K12_EMPTY || old == i) return h;
        h = (h + 1) & (K12_SLOTS - 1);
    }
    return K12_EMPTY;
}
static_assert(K12_SLOTS == 512, "k12_slot's shift");
// p may point to LDS or to device memory; a field with nothing to add is skipped
__device__ __forceinline__ void k12_add(u64* p, u64 x) { if (x) atomicAdd(p, x); }
__device__ __forceinline__ void k12_add(u32* p, u32 x) { if (x) atomicAdd(p, x); }
__device__ __forceinline__ void k12_max(u64* p, u64 x) { if (x) atomicMax(p, x); }
// the u64 words of an incident row: count, err, sum_ns, score_q32, rank_sum
__device__ __forceinline__ u64* k12_w(sg_incident_out* o) { return reinterpret_cast<u64*>(o); }

// The wave fold of both folding passes: i is the lane's incident (SG_NO_INCIDENT: none).  false: no lane of the wave has one.
// Else `one` says whether every lane that has one names the same, and the return value whether this lane carries a contribution
// to the table: with `one` the wave's lead lane (the caller reduces the wave's values in registers first), else every lane that
// has an incident.  Called by whole waves.
__device__ __forceinline__ bool k12_wave(u32 i, bool& one, bool& mine) {
    const bool act = i != SG_NO_INCIDENT;
    const u64 m = __ballot(act);
    if (!m) return false;
    const u32 lead = (u32)(__ffsll((long long)m) - 1);
    const u32 i0 = __shfl(i, lead, 64);
    one = __ballot(act && i != i0) == 0;
    mine = one ? (threadIdx.x & 63) == lead : act;
    return true;
}

template <class S>
__device__ __forceinline__ void k12_nodes_t(const typename S::Args& a) {
    __shared__ u32 key[K12_SLOTS], cnt[K12_SLOTS];
    __shared__ u64 top[K12_SLOTS], rsum[K12_SLOTS], rmax[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) { key[s] = K12_EMPTY; cnt[s] = 0; top[s] = 0; rsum[s] = 0; rmax[s] = 0; }
    __syncthreads();
    const u64 N = S::nodes(a), stride = (u64)gridDim.x * K12_THREADS;
    for (u64 vb = (u64)blockIdx.x * K12_THREADS; vb < N; vb += stride) {   // (uniform per wave: the wave reductions see 64 lanes)
        const u64 v = vb + t;
        u32 i = SG_NO_INCIDENT;
        u64 tk = 0, rk = 0;
        if (v < N) {
            u32 k;
            if (S::index(a, v, k)) {
                if (a.flag[k]) i = a.num[a.lab[k]];
                S::keep(a, k, i);
            }
            a.node_inc[v] = i;
            if (i != SG_NO_INCIDENT) {
                tk = ((u64)k9_score_key(a.nodes[v].score) << 32) | (u64)(~(u32)v);
                if (a.rank) rk = a.rank[v].rank;
            }
        }
        bool one, mine;
        if (!k12_wave(i, one, mine)) continue;
        u32 c = i != SG_NO_INCIDENT ? 1u : 0u;
        u64 rs = rk, rm = rk;
        if (one) { c = wave_sum_u32(c); tk = wave_max_u64(tk); rs = wave_sum_u64(rs); rm = wave_max_u64(rm); }
        if (mine) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k12_add(&cnt[s], c); k12_max(&top[s], tk); k12_add(&rsum[s], rs); k12_max(&rmax[s], rm); }
            else { k12_add(&a.out[i].nodes, c); k12_max(&a.keys[i].top, tk); k12_add(k12_w(a.out + i) + 4, rs); k12_max(&a.keys[i].rmax, rm); }
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        k12_add(&a.out[i].nodes, cnt[s]); k12_max(&a.keys[i].top, top[s]); k12_add(k12_w(a.out + i) + 4, rsum[s]); k12_max(&a.keys[i].rmax, rmax[s]);
    }
}

template <class S>
__device__ __forceinline__ void k12_rows_t(const typename S::Args& a) {
    __shared__ u32 key[K12_SLOTS], edg[K12_SLOTS];
    __shared__ u64 cnt[K12_SLOTS], err[K12_SLOTS], sum[K12_SLOTS], q32[K12_SLOTS], worst[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) { key[s] = K12_EMPTY; edg[s] = 0; cnt[s] = 0; err[s] = 0; sum[s] = 0; q32[s] = 0; worst[s] = 0; }
    __syncthreads();
    const u64 E = S::rows(a), stride = (u64)gridDim.x * K12_THREADS;
    for (u64 jb = (u64)blockIdx.x * K12_THREADS; jb < E; jb += stride) {   // (uniform per wave)
        const u64 j = jb + t;
        u32 i = SG_NO_INCIDENT;
        u64 xc = 0, xe = 0, xs = 0, xq = 0, xw = 0;
        if (j < E) i = S::row(a, j, xc, xe, xs, xq, xw);
        bool one, mine;
        if (!k12_wave(i, one, mine)) continue;
        u32 n = i != SG_NO_INCIDENT ? 1u : 0u;
        if (one) { n = wave_sum_u32(n); xc = wave_sum_u64(xc); xe = wave_sum_u64(xe); xs = wave_sum_u64(xs); xq = wave_sum_u64(xq); xw = wave_max_u64(xw); }
        if (mine) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k12_add(&edg[s], n); k12_add(&cnt[s], xc); k12_add(&err[s], xe); k12_add(&sum[s], xs); k12_add(&q32[s], xq); k12_max(&worst[s], xw); }
            else {
                sg_incident_out* o = a.out + i;
                k12_add(&o->edges, n); k12_add(k12_w(o), xc); k12_add(k12_w(o) + 1, xe); k12_add(k12_w(o) + 2, xs); k12_add(k12_w(o) + 3, xq);
                k12_max(&a.keys[i].worst, xw);
            }
        }
    }
    // the culprit: the smallest node row whose rank is its incident's largest (the nodes pass, the launch before, found that)
    if (a.rank) {
        const u64 N = S::nodes(a);
        for (u64 v = (u64)blockIdx.x * K12_THREADS + t; v < N; v += stride) {
            const u32 i = a.node_inc[v];
            if (i != SG_NO_INCIDENT && a.rank[v].rank == a.keys[i].rmax) atomicMin(&a.out[i].culprit_node, (u32)v);
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        sg_incident_out* o = a.out + i;
        k12_add(&o->edges, edg[s]); k12_add(k12_w(o), cnt[s]); k12_add(k12_w(o) + 1, err[s]); k12_add(k12_w(o) + 2, sum[s]); k12_add(k12_w(o) + 3, q32[s]);
        k12_max(&a.keys[i].worst, worst[s]);
    }
}

// (an incident has a red row and a node: both keys were written)
__device__ __forceinline__ void k12_finish_t(const K12Keys* keys, sg_incident_out* out, const u64* count) {
    const u64 I = *count;
    for (u64 i = (u64)blockIdx.x * K12_THREADS + threadIdx.x; i < I; i += (u64)gridDim.x * K12_THREADS) {
        const K12Keys k = keys[i];
        sg_incident_out* o = out + i;
        o->value_max = k9_key_score((u32)(k.worst >> 32)); o->worst_row = ~(u32)k.worst;
        o->top_node = ~(u32)k.top;
    }
}

__global__ __launch_bounds__(K12_THREADS) void k12_label(IncArgs a) { k12_label_t<K12Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k12_number(IncArgs a) { k12_number_t<K12Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k12_nodes(IncArgs a) { k12_nodes_t<K12Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k12_rows(IncArgs a) { k12_rows_t<K12Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k12_finish(IncArgs a) { k12_finish_t(a.keys, a.out, a.nd.count); }
