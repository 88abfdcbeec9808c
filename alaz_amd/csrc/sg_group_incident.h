// sg_group_incident.h — K18: each window's anomalous group edges grouped into workload incidents on the device
// (include/servicegraph.h, "workload incidents").  Included after sg_group_rank.h: it reuses K12's union-find (k12_ld, k12_find,
// k12_unite), K12's folding helpers (k12_slot, k12_add, k12_max, k12_w, K12Keys), K16's group key (k16_gk, k16_edges_of), K9's keys
// (k9_score_key, k9_key_score, k9_worst_key), sg_nodes_of, the wave reductions, block_excl_scan and k9_scan unchanged, and adds
// kernels of its own.
//
// K12's definition with "row" read as "group edge" and "node row" read as "workload row".  K12 works in K9's node-key space; K16's
// rows are dense and ascending by group key, so this stage works in ROW-INDEX space as K17 does: every per-node array is [NC] by
// row position and is read coalesced.  parent[v] <= v then makes a component's root its smallest row, which is first_node itself:
// K12's kinc[key] detour is gone, node_inc[v] serves the rows pass.  pos is the stage's own (K17 is optional; its table cannot be
// borrowed); only the window's keys of pos are written and only those are read, so nothing is zeroed between windows.  Every field
// of an incident is an integer sum, an integer max or the max of a 64-bit key (order-preserving bits << 32 | ~index): the result
// has one value whatever order the workgroups and lanes run in.  Eight plain launches on the window's stream; no workgroup ever
// waits for another: the only loops over shared state are CAS retries (another hook succeeded) and root walks (parent[x] < x).
//
//   k18_init    per workload row v: pos[gk(ref_v)] = v, parent[v] = v, flag[v] = 0
//   k18_hook    per group edge j: two 16-byte loads of the 80-byte row (from | to; score_max in the last word), the row positions
//               through pos, the red test; red: flag both rows and k12_unite them.  esrc[j] = the source's row position, SG_NONE for
//               a group edge that is not red: the rows pass repeats neither the lookups nor the test.  Every access to parent[] in
//               this launch is K12's agent-scope relaxed atomic (the CUs' L1s are not coherent inside a launch)
//   k18_label   per workload row (a later launch: plain loads): lab[v] = root(v); heads (flagged and lab == v) counted per workgroup
//   k9_scan     (1 workgroup, K9's kernel) exclusive scan of the counts; the incident count of the window
//   k18_number  per workload row: a head's incident number is its exclusive rank: num[v]; the incident's row and keys start here
//   k18_nodes   per workload row: node_inc[v]; nodes, the top row's key, rank_sum and the largest rank folded per incident
//   k18_rows    per group edge with esrc[j] != SG_NONE, under node_inc[esrc[j]]: edges, count, err, sum_ns, score_q32, the worst
//               group edge's key; beside it per workload row: culprit_node = the smallest row whose rank is the incident's largest
//   k18_finish  per incident: value_max / worst_row and top_node out of their keys
//
// The two folding passes keep K12's shape: a wave whose active lanes all name one incident (group edges ascend by source: the
// common case) reduces in registers first, every contribution then goes to the K12_SLOTS-slot LDS table, and a workgroup adds its
// table to device memory once per field and distinct incident; only an incident without a slot after K12_PROBES probes is added to
// device memory directly.
#pragma once

#define K18_THREADS 256
#define K18_MAX_WGS 1024          // node workgroups at most (k9_scan scans one count per thread)

static_assert(K18_THREADS == K12_THREADS, "the folding passes zero and add K12's LDS table with K12's stride");
static_assert(K18_MAX_WGS == K9_MAX_WGS && K18_MAX_WGS <= K9_SCAN_THREADS, "k9_scan scans K18's head counts");
static_assert(offsetof(sg_group_edge, from_ref) == 48 && offsetof(sg_group_edge, to_ref) == 52 && offsetof(sg_group_edge, score_max) == 76 &&
              offsetof(sg_group_edge, err_count) == 8 && offsetof(sg_group_edge, sum_ns) == 16 && sizeof(sg_group_edge) == 80,
              "k18_hook and k18_rows read sg_group_edge by 16-byte word");

struct GroupIncArgs {
    GroupNodesArgs g;             // K16's part: the id spaces, max_edges, groups, gcount, max_groups, gk, nc (k16_gk, k16_edges_of);
                                  // g.nd.blk, g.nd.count: k9_scan's (the head counts in, their scan and the incident count out)
    const sg_node_out* nodes;     // the window's workload rows
    const u64* ncount;            // their count
    const sg_edge_trend* trend;   // the window's group trend rows (a trend key), else unused
    const sg_node_rank* rank;     // the window's workload rank rows, NULL with the workload ranking off
    u32 by; float min_value;
    u32 node_per;                 // workload rows per workgroup of k18_label / k18_number (a multiple of K18_THREADS)
    u32* pos;                     // [GK] row position by group key (the window's keys only)
    u32* parent; u32* flag; u32* lab; u32* num;   // [NC] by row position
    u32* esrc;                    // [max_edges] the source's row position of a red group edge, else SG_NONE
    K12Keys* keys;                // [NC] by incident
    sg_incident_out* out;         // [NC] this window's incidents (g.nd.count: their count)
    u32* node_inc;                // [NC] this window's incident per workload row
};

__device__ __forceinline__ u64 k18_rows_of(const GroupIncArgs& a) { return sg_nodes_of(a.ncount, a.g.nc); }
// the value of group edge j (score_max: the last word of its row)
__device__ __forceinline__ float k18_value(const GroupIncArgs& a, u64 j, float score_max) {
    return a.by == SG_SEL_SCORE ? score_max : a.by == SG_SEL_LAT_DEV ? a.trend[j].lat_dev : a.trend[j].err_dev;
}

__global__ __launch_bounds__(K18_THREADS) void k18_init(GroupIncArgs a) {
    const u64 N = k18_rows_of(a);
    for (u64 v = (u64)blockIdx.x * K18_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K18_THREADS) {
        const u32 k = k16_gk(a.g, a.nodes[v].ref);
        if (k != SG_NONE && k < a.g.gk) a.pos[k] = (u32)v;           // (cannot fail: K16 made the row from such a key)
        a.parent[v] = (u32)v; a.flag[v] = 0;
    }
}

__global__ __launch_bounds__(K18_THREADS) void k18_hook(GroupIncArgs a) {
    const u64 G = k16_edges_of(a.g), N = k18_rows_of(a);
    for (u64 j = (u64)blockIdx.x * K18_THREADS + threadIdx.x; j < G; j += (u64)gridDim.x * K18_THREADS) {
        const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.g.groups + j);   // word 3: from | to << 32, ..; word 4: .., worst_row | score_max << 32
        const ulonglong2 w3 = r[3], w4 = r[4];
        const u32 fk = k16_gk(a.g, (u32)w3.x), tk = k16_gk(a.g, (u32)(w3.x >> 32));
        u32 src = SG_NONE;
        if (fk != SG_NONE && tk != SG_NONE && fk < a.g.gk && tk < a.g.gk) {   // (a ref beyond the id spaces has no row: never red)
            const u32 s = a.pos[fk], d = a.pos[tk];
            if (s < N && d < N && k18_value(a, j, __uint_as_float((u32)(w4.y >> 32))) >= a.min_value) {   // (a row cut at the capacity has no position)
                src = s;
                a.flag[s] = 1; a.flag[d] = 1;                         // (every writer stores 1; read by the next launch)
                if (s != d) k12_unite(a.parent, s, d);                // (its loops: a CAS retry means another hook succeeded, and at most N - 1 hooks
                                                                      //  ever succeed; k12_find's walk strictly descends: parent[x] < x off a root)
            }
        }
        a.esrc[j] = src;
    }
}

// the workgroup's workload rows [v0, v1) in rounds of K18_THREADS
__device__ __forceinline__ void k18_node_span(const GroupIncArgs& a, u64 N, u64& v0, u64& v1) {
    v0 = (u64)blockIdx.x * a.node_per; v1 = v0 + a.node_per;
    if (v0 > N) v0 = N;
    if (v1 > N) v1 = N;
}

__global__ __launch_bounds__(K18_THREADS) void k18_label(GroupIncArgs a) {
    __shared__ u32 ws[K18_THREADS / 64];
    const u32 t = threadIdx.x;
    u64 v0, v1; k18_node_span(a, k18_rows_of(a), v0, v1);
    u32 c = 0;
    for (u64 v = v0 + t; v < v1; v += K18_THREADS) {
        u32 x = (u32)v;
        for (u32 p = a.parent[x]; p != x; p = a.parent[x]) x = p;    // (strictly descending, p < x: it ends at a root after at most v steps)
        a.lab[v] = x;
        c += (x == (u32)v && a.flag[v]) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if ((t & 63) == 0) ws[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        u32 s = 0;
        for (int w = 0; w < K18_THREADS / 64; w++) s += ws[w];
        a.g.nd.blk[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(K18_THREADS) void k18_number(GroupIncArgs a) {
    __shared__ u32 wsum[K18_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    u64 v0, v1; k18_node_span(a, k18_rows_of(a), v0, v1);
    u32 base = a.g.nd.blk[K18_MAX_WGS + blockIdx.x];
    for (u64 vb = v0; vb < v1; vb += K18_THREADS) {                 // (uniform: every thread takes every round)
        const u64 v = vb + t;
        const bool head = v < v1 && a.lab[v] == (u32)v && a.flag[v];
        u32 tot;
        const u32 x = block_excl_scan<K18_THREADS>(head ? 1u : 0u, wsum, &tot);
        if (head) {
            const u32 i = base + x;
            a.num[v] = i;
            sg_incident_out o{};
            o.first_node = (u32)v; o.worst_row = SG_NO_INCIDENT; o.top_node = SG_NO_INCIDENT; o.culprit_node = SG_NO_INCIDENT;
            a.out[i] = o;
            K12Keys z; z.worst = z.top = z.rmax = 0;
            a.keys[i] = z;
        }
        base += tot;
    }
}

__global__ __launch_bounds__(K18_THREADS) void k18_nodes(GroupIncArgs a) {
    __shared__ u32 key[K12_SLOTS], cnt[K12_SLOTS];
    __shared__ u64 top[K12_SLOTS], rsum[K12_SLOTS], rmax[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K18_THREADS) { key[s] = K12_EMPTY; cnt[s] = 0; top[s] = 0; rsum[s] = 0; rmax[s] = 0; }
    __syncthreads();
    const u64 N = k18_rows_of(a), stride = (u64)gridDim.x * K18_THREADS;
    for (u64 vb = (u64)blockIdx.x * K18_THREADS; vb < N; vb += stride) {   // (uniform per wave: the wave reductions see 64 lanes)
        const u64 v = vb + t;
        u32 i = SG_NO_INCIDENT;
        u64 tk = 0, rk = 0;
        if (v < N) {
            if (a.flag[v]) i = a.num[a.lab[v]];
            a.node_inc[v] = i;
            if (i != SG_NO_INCIDENT) {
                tk = ((u64)k9_score_key(a.nodes[v].score) << 32) | (u64)(~(u32)v);
                if (a.rank) rk = a.rank[v].rank;
            }
        }
        const bool act = i != SG_NO_INCIDENT;
        const u64 m = __ballot(act);
        if (!m) continue;
        const u32 lead = (u32)(__ffsll((long long)m) - 1);
        const u32 i0 = __shfl(i, lead, 64);
        const bool one = __ballot(act && i != i0) == 0;              // every active lane names one incident
        u32 c = act ? 1u : 0u;
        u64 rs = rk, rm = rk;
        if (one) { c = wave_sum_u32(c); tk = wave_max_u64(tk); rs = wave_sum_u64(rs); rm = wave_max_u64(rm); }
        if (one ? (t & 63) == lead : act) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k12_add(&cnt[s], c); k12_max(&top[s], tk); k12_add(&rsum[s], rs); k12_max(&rmax[s], rm); }
            else { k12_add(&a.out[i].nodes, c); k12_max(&a.keys[i].top, tk); k12_add(k12_w(a.out + i) + 4, rs); k12_max(&a.keys[i].rmax, rm); }
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K18_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        k12_add(&a.out[i].nodes, cnt[s]); k12_max(&a.keys[i].top, top[s]); k12_add(k12_w(a.out + i) + 4, rsum[s]); k12_max(&a.keys[i].rmax, rmax[s]);
    }
}

__global__ __launch_bounds__(K18_THREADS) void k18_rows(GroupIncArgs a) {
    __shared__ u32 key[K12_SLOTS], edg[K12_SLOTS];
    __shared__ u64 cnt[K12_SLOTS], err[K12_SLOTS], sum[K12_SLOTS], q32[K12_SLOTS], worst[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K18_THREADS) { key[s] = K12_EMPTY; edg[s] = 0; cnt[s] = 0; err[s] = 0; sum[s] = 0; q32[s] = 0; worst[s] = 0; }
    __syncthreads();
    const u64 G = k16_edges_of(a.g), stride = (u64)gridDim.x * K18_THREADS;
    for (u64 jb = (u64)blockIdx.x * K18_THREADS; jb < G; jb += stride) {   // (uniform per wave)
        const u64 j = jb + t;
        u32 i = SG_NO_INCIDENT;
        u64 xc = 0, xe = 0, xs = 0, xq = 0, xw = 0;
        if (j < G) {
            const u32 s = a.esrc[j];
            if (s != SG_NONE) {                                       // (red: k18_hook flagged s, so node_inc[s] is an incident)
                const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.g.groups + j);   // count, err_count | sum_ns, .. | .., score_q32 | .. | .., worst_row | score_max << 32
                const ulonglong2 w0 = r[0];
                i = a.node_inc[s];
                xc = w0.x; xe = w0.y; xs = r[1].x; xq = r[2].y;
                xw = k9_worst_key(k18_value(a, j, __uint_as_float((u32)(r[4].y >> 32))), j);
            }
        }
        const bool act = i != SG_NO_INCIDENT;
        const u64 m = __ballot(act);
        if (!m) continue;
        const u32 lead = (u32)(__ffsll((long long)m) - 1);
        const u32 i0 = __shfl(i, lead, 64);
        const bool one = __ballot(act && i != i0) == 0;
        u32 n = act ? 1u : 0u;
        if (one) { n = wave_sum_u32(n); xc = wave_sum_u64(xc); xe = wave_sum_u64(xe); xs = wave_sum_u64(xs); xq = wave_sum_u64(xq); xw = wave_max_u64(xw); }
        if (one ? (t & 63) == lead : act) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k12_add(&edg[s], n); k12_add(&cnt[s], xc); k12_add(&err[s], xe); k12_add(&sum[s], xs); k12_add(&q32[s], xq); k12_max(&worst[s], xw); }
            else {
                sg_incident_out* o = a.out + i;
                k12_add(&o->edges, n); k12_add(k12_w(o), xc); k12_add(k12_w(o) + 1, xe); k12_add(k12_w(o) + 2, xs); k12_add(k12_w(o) + 3, xq);
                k12_max(&a.keys[i].worst, xw);
            }
        }
    }
    // the culprit: the smallest workload row whose rank is its incident's largest (k18_nodes, the launch before, found that)
    if (a.rank) {
        const u64 N = k18_rows_of(a);
        for (u64 v = (u64)blockIdx.x * K18_THREADS + t; v < N; v += stride) {
            const u32 i = a.node_inc[v];
            if (i != SG_NO_INCIDENT && a.rank[v].rank == a.keys[i].rmax) atomicMin(&a.out[i].culprit_node, (u32)v);
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K18_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        sg_incident_out* o = a.out + i;
        k12_add(&o->edges, edg[s]); k12_add(k12_w(o), cnt[s]); k12_add(k12_w(o) + 1, err[s]); k12_add(k12_w(o) + 2, sum[s]); k12_add(k12_w(o) + 3, q32[s]);
        k12_max(&a.keys[i].worst, worst[s]);
    }
}

__global__ __launch_bounds__(K18_THREADS) void k18_finish(GroupIncArgs a) {
    const u64 I = *a.g.nd.count;
    for (u64 i = (u64)blockIdx.x * K18_THREADS + threadIdx.x; i < I; i += (u64)gridDim.x * K18_THREADS) {
        const K12Keys k = a.keys[i];
        sg_incident_out* o = a.out + i;
        o->value_max = k9_key_score((u32)(k.worst >> 32)); o->worst_row = ~(u32)k.worst;   // (an incident has a red group edge and a row)
        o->top_node = ~(u32)k.top;
    }
}
