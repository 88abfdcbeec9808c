// sg_group_incident.h — K18: each window's anomalous group edges grouped into workload incidents on the device
// (include/servicegraph.h, "workload incidents").  Included after sg_group_rank.h: K12's passes from the label pass on
// (sg_incident.h: k12_label_t, k12_number_t, k12_nodes_t, k12_rows_t, k12_finish_t) over the space policy K18Space below, K12's
// union-find (k12_unite), K16's group key (k16_gk, k16_edges_of), K9's keys (k9_worst_key), sg_nodes_of and k9_scan; its own are
// the first two passes, the policy and the kernels' names.
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
// The two folding passes are K12's (group edges ascend by source: a wave that names one incident is the common case here too).
#pragma once

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
    u32 node_per;                 // workload rows per workgroup of k18_label / k18_number (a multiple of K12_THREADS)
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

__global__ __launch_bounds__(K12_THREADS) void k18_init(GroupIncArgs a) {
    const u64 N = k18_rows_of(a);
    for (u64 v = (u64)blockIdx.x * K12_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K12_THREADS) {
        const u32 k = k16_gk(a.g, a.nodes[v].ref);
        if (k != SG_NONE && k < a.g.gk) a.pos[k] = (u32)v;           // (cannot fail: K16 made the row from such a key)
        a.parent[v] = (u32)v; a.flag[v] = 0;
    }
}

__global__ __launch_bounds__(K12_THREADS) void k18_hook(GroupIncArgs a) {
    const u64 G = k16_edges_of(a.g), N = k18_rows_of(a);
    for (u64 j = (u64)blockIdx.x * K12_THREADS + threadIdx.x; j < G; j += (u64)gridDim.x * K12_THREADS) {
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

// K18's space: every per-node array is indexed by row position, and node_inc[v] itself serves the rows pass through esrc[j]
struct K18Space {
    typedef GroupIncArgs Args;
    static __device__ __forceinline__ u64 nodes(const GroupIncArgs& a) { return k18_rows_of(a); }
    static __device__ __forceinline__ u64 rows(const GroupIncArgs& a) { return k16_edges_of(a.g); }
    static __device__ __forceinline__ bool index(const GroupIncArgs&, u64 v, u32& k) { k = (u32)v; return true; }
    static __device__ __forceinline__ const NodesArgs& scan(const GroupIncArgs& a) { return a.g.nd; }
    static __device__ __forceinline__ void keep(const GroupIncArgs&, u32, u32) {}
    // group edge j's incident, SG_NO_INCIDENT unless k18_hook found it red, and what it adds (k18_hook flagged esrc[j], so
    // node_inc of it is an incident)
    static __device__ __forceinline__ u32 row(const GroupIncArgs& a, u64 j, u64& xc, u64& xe, u64& xs, u64& xq, u64& xw) {
        const u32 s = a.esrc[j];
        if (s == SG_NONE) return SG_NO_INCIDENT;
        const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.g.groups + j);   // count, err_count | sum_ns, .. | .., score_q32 | .. | .., worst_row | score_max << 32
        const ulonglong2 w0 = r[0];
        xc = w0.x; xe = w0.y; xs = r[1].x; xq = r[2].y;
        xw = k9_worst_key(k18_value(a, j, __uint_as_float((u32)(r[4].y >> 32))), j);
        return a.node_inc[s];
    }
};

__global__ __launch_bounds__(K12_THREADS) void k18_label(GroupIncArgs a) { k12_label_t<K18Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k18_number(GroupIncArgs a) { k12_number_t<K18Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k18_nodes(GroupIncArgs a) { k12_nodes_t<K18Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k18_rows(GroupIncArgs a) { k12_rows_t<K18Space>(a); }
__global__ __launch_bounds__(K12_THREADS) void k18_finish(GroupIncArgs a) { k12_finish_t(a.keys, a.out, a.g.nd.count); }
