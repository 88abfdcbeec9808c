// sg_group_impact.h — K22: the upstream impact of each workload incident on the device (include/servicegraph.h, "workload impact").
// Included after sg_group_incident.h: K16's group key and row counts (k16_gk, k16_edges_of, sg_nodes_of), K12's LDS table
// (k12_slot, k12_add, k12_max over K12_SLOTS) and its thread count; the kernels are its own.
//
// Who depends on incident i, and how much traffic entered the system through workloads upstream of it?  A CALL EDGE is a group edge
// with count > 0 whose two refs have workload rows u != v ("u calls v"); d_i(x) is the fewest call edges on a directed path from row
// x to a member of incident i.  The stage is a breadth-first search against the call edges from the members of up to 64 W incidents
// at once, W = ceil(max_incidents / 64) u64 words per workload row, cut at max_hops rounds.  Work is in ROW-INDEX space as K17's and
// K18's; pos is the stage's own.  Of K18 it reads only what the window's slot owns: the incident count and the incident per workload
// row (K18's pos and esrc belong to whichever window ran K18 last).  Every field is an integer sum or the max of a 64-bit key: the
// result has one value whatever order the workgroups and lanes run in.  2 max_hops + 4 plain launches on the window's stream; no
// workgroup ever waits for another, and nothing is exchanged inside a launch: a round's bits are written by one launch and read by
// the next.
//
//   k22_seed    per workload row v: pos[gk(ref_v)] = v; have[v] = fresh[v] = 0; next[v] = the bit of the row's incident, if covered;
//               arrive[v] = 0; hops[v] = SG_NO_HOPS.  Beside it: every impact row and the round counters zeroed
//   k22_ends    per group edge j: ends[j] = s | d << 32 by row position, all ones for a group edge that is no call edge; arrive[d] = 1
//               ("a call edge arrives here": d is no entry row); INTO_COUNT / INTO_ERR folded under inc[d] when inc[s] differs.  The
//               rounds read these 8 bytes, not the 80-byte rows, and repeat no lookup
//   k22_pull    round r = 0 .. max_hops, per workload row: new = next & ~have; have |= new; fresh = new; next = 0.  A row with new
//               bits takes hops = min(hops, r) and folds, per new bit, the impact row of that incident: ENTRIES / ENTRY_COUNT /
//               ENTRY_ERR for an entry row (every round: the members are round 0), EXPOSED and the FAR key r << 32 | ~v for r >= 1,
//               DIRECT for r == 1.  The rows that got new bits are counted into cnt[r].  Round r >= 1 returns on one uniform load when
//               round r - 1 counted none (k22_push did nothing then, and every fresh word is already 0)
//   k22_push    round r = 1 .. max_hops, per call edge: returns likewise; else next[s] |= fresh[d], 64-bit atomics, zero words skipped
//   k22_finish  per covered incident: the FAR key into its word; the covered count
//
// fresh and next are separate, so a bit moves exactly one hop per round: k22_push reads only what k22_pull published one launch
// earlier.  The folds go through K12's LDS table, flushed once per workgroup, with K12's direct fallback when no slot is found.
// (Not kept: combining the lanes of a wave that share s before k22_push's atomic — group edges ascend by source, so it would save
// atomics, but it is a segmented wave scan per mask word against one global atomic per non-zero word.)
#pragma once

static_assert(SG_IMPACT_WORDS == 8 && SG_IMPACT_MAX_INCIDENTS % 64 == 0 && SG_NO_HOPS == 0xFFFFFFFFu, "the impact row and the mask words");
static_assert(offsetof(sg_node_out, out_count) == 0 && offsetof(sg_node_out, out_err) == 16 && offsetof(sg_node_out, ref) == 96,
              "k22_seed and k22_pull read sg_node_out by field");

#define K22_NO_EDGE 0xFFFFFFFFFFFFFFFFull   // ends[j] of a group edge that is no call edge

struct ImpactArgs {
    GroupNodesArgs g;             // K16's part: the id spaces, max_edges, groups, gcount, max_groups, gk, nc (k16_gk, k16_edges_of)
    const sg_node_out* nodes;     // the window's workload rows
    const u64* ncount;            // their count
    const u64* icount;            // K18's slot: the window's incident count
    const u32* node_inc;          //             and its incident per workload row
    u32 max_inc, max_hops, W;     // W = ceil(max_inc / 64) mask words per workload row
    u32* pos;                     // [GK] row position by group key (the window's keys only)
    u64* fresh; u64* next;        // [NC][W] the bits a row got last round; the bits pushed to it for the next
    u64* ends;                    // [max_edges] s | d << 32 of a call edge, else K22_NO_EDGE
    u32* arrive;                  // [NC] 1: a call edge arrives at the row
    u32* cnt;                     // [SG_IMPACT_MAX_HOPS + 1] rows that got new bits, by round
    u64* have;                    // [NC][W] this window's mask rows
    u64* out;                     // [max_inc][SG_IMPACT_WORDS] this window's impact rows
    u32* hops;                    // [NC] this window's hops per workload row
    u64* count;                   // this window's covered incidents
};

__device__ __forceinline__ u64 k22_rows_of(const ImpactArgs& a) { return sg_nodes_of(a.ncount, a.g.nc); }
// the covered incidents: the first min(I, max_incidents)
__device__ __forceinline__ u32 k22_covered(const ImpactArgs& a) {
    const u64 I = sg_nodes_of(a.icount, a.g.nc);
    return I < a.max_inc ? (u32)I : a.max_inc;
}

__global__ __launch_bounds__(K12_THREADS) void k22_seed(ImpactArgs a) {
    const u64 N = k22_rows_of(a), g0 = (u64)blockIdx.x * K12_THREADS + threadIdx.x, stride = (u64)gridDim.x * K12_THREADS;
    const u32 cov = k22_covered(a), W = a.W;
    for (u64 v = g0; v < N; v += stride) {
        const u32 k = k16_gk(a.g, a.nodes[v].ref);
        if (k != SG_NONE && k < a.g.gk) a.pos[k] = (u32)v;           // (cannot fail: K16 made the row from such a key)
        const u32 i = a.node_inc[v];
        for (u32 w = 0; w < W; w++) {
            const u64 x = v * W + w;
            a.have[x] = 0; a.fresh[x] = 0;
            a.next[x] = (i < cov && (i >> 6) == w) ? 1ull << (i & 63u) : 0;
        }
        a.arrive[v] = 0; a.hops[v] = SG_NO_HOPS;
    }
    for (u64 x = g0; x < (u64)a.max_inc * SG_IMPACT_WORDS; x += stride) a.out[x] = 0;
    for (u64 r = g0; r <= SG_IMPACT_MAX_HOPS; r += stride) a.cnt[r] = 0;
}

__global__ __launch_bounds__(K12_THREADS) void k22_ends(ImpactArgs a) {
    __shared__ u32 key[K12_SLOTS];
    __shared__ u64 ic[K12_SLOTS], ie[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) { key[s] = K12_EMPTY; ic[s] = 0; ie[s] = 0; }
    __syncthreads();
    const u64 G = k16_edges_of(a.g), N = k22_rows_of(a);
    const u32 cov = k22_covered(a);
    for (u64 j = (u64)blockIdx.x * K12_THREADS + t; j < G; j += (u64)gridDim.x * K12_THREADS) {
        const ulonglong2* r = reinterpret_cast<const ulonglong2*>(a.g.groups + j);   // word 0: count, err_count; word 3: from | to << 32, ..
        const ulonglong2 w0 = r[0];
        const u64 ft = r[3].x;
        const u32 fk = k16_gk(a.g, (u32)ft), tk = k16_gk(a.g, (u32)(ft >> 32));
        u64 e = K22_NO_EDGE;
        if (w0.x && fk != SG_NONE && tk != SG_NONE && fk < a.g.gk && tk < a.g.gk) {   // (count == 0: an alive-only group edge)
            const u32 s = a.pos[fk], d = a.pos[tk];
            if (s < N && d < N && s != d) {                           // (a row cut at the capacity has no position)
                e = (u64)s | (u64)d << 32;
                a.arrive[d] = 1;                                      // (every writer stores 1; read by the next launch)
                const u32 i = a.node_inc[d];
                if (i < cov && a.node_inc[s] != i) {
                    const u32 sl = k12_slot(key, i);
                    if (sl != K12_EMPTY) { k12_add(&ic[sl], w0.x); k12_add(&ie[sl], w0.y); }
                    else { k12_add(a.out + (u64)i * SG_IMPACT_WORDS + SG_IMPACT_INTO_COUNT, w0.x); k12_add(a.out + (u64)i * SG_IMPACT_WORDS + SG_IMPACT_INTO_ERR, w0.y); }
                }
            }
        }
        a.ends[j] = e;
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        k12_add(a.out + (u64)i * SG_IMPACT_WORDS + SG_IMPACT_INTO_COUNT, ic[s]); k12_add(a.out + (u64)i * SG_IMPACT_WORDS + SG_IMPACT_INTO_ERR, ie[s]);
    }
}

__global__ __launch_bounds__(K12_THREADS) void k22_pull(ImpactArgs a, u32 r) {
    if (r && a.cnt[r - 1] == 0) return;                               // (uniform: nothing was pushed, and every fresh word is 0 already)
    __shared__ u32 key[K12_SLOTS], ex[K12_SLOTS], di[K12_SLOTS], en[K12_SLOTS], rows;
    __shared__ u64 ec[K12_SLOTS], ee[K12_SLOTS], far[K12_SLOTS];
    const u32 t = threadIdx.x, W = a.W;
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) { key[s] = K12_EMPTY; ex[s] = 0; di[s] = 0; en[s] = 0; ec[s] = 0; ee[s] = 0; far[s] = 0; }
    if (t == 0) rows = 0;
    __syncthreads();
    const u64 N = k22_rows_of(a), stride = (u64)gridDim.x * K12_THREADS;
    const u32 exposed = r ? 1u : 0u, direct = r == 1 ? 1u : 0u;
    for (u64 vb = (u64)blockIdx.x * K12_THREADS; vb < N; vb += stride) {   // (uniform per wave: the ballot sees 64 lanes)
        const u64 v = vb + t;
        bool any = false;
        if (v < N) {
            for (u32 w = 0; w < W; w++) {
                const u64 x = v * W + w;
                const u64 nx = a.next[x], fo = a.fresh[x];
                u64 nw = 0;
                if (nx) {
                    const u64 hv = a.have[x];
                    nw = nx & ~hv;
                    a.next[x] = 0;
                    if (nw) a.have[x] = hv | nw;
                }
                if (fo != nw) a.fresh[x] = nw;
                if (!nw) continue;
                any = true;
                const bool entry = a.arrive[v] == 0;
                const u64 oc = entry ? a.nodes[v].out_count : 0, oe = entry ? a.nodes[v].out_err : 0;
                const u64 fk = exposed ? (u64)r << 32 | (u64)(~(u32)v) : 0;
                while (nw) {
                    const u32 i = w * 64u + (u32)(__ffsll((long long)nw) - 1);
                    nw &= nw - 1;
                    const u32 sl = k12_slot(key, i);
                    if (sl != K12_EMPTY) {
                        k12_add(&ex[sl], exposed); k12_add(&di[sl], direct); k12_max(&far[sl], fk);
                        if (entry) { k12_add(&en[sl], 1u); k12_add(&ec[sl], oc); k12_add(&ee[sl], oe); }
                    } else {
                        u64* o = a.out + (u64)i * SG_IMPACT_WORDS;
                        k12_add(o + SG_IMPACT_EXPOSED, (u64)exposed); k12_add(o + SG_IMPACT_DIRECT, (u64)direct); k12_max(o + SG_IMPACT_FAR, fk);
                        if (entry) { k12_add(o + SG_IMPACT_ENTRIES, (u64)1); k12_add(o + SG_IMPACT_ENTRY_COUNT, oc); k12_add(o + SG_IMPACT_ENTRY_ERR, oe); }
                    }
                }
            }
            if (any && r < a.hops[v]) a.hops[v] = r;
        }
        const u64 m = __ballot(any);
        if (m && (t & 63) == 0) atomicAdd(&rows, (u32)__popcll(m));
    }
    __syncthreads();
    if (t == 0 && rows) atomicAdd(a.cnt + r, rows);
    for (u32 s = t; s < K12_SLOTS; s += K12_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        u64* o = a.out + (u64)i * SG_IMPACT_WORDS;
        k12_add(o + SG_IMPACT_EXPOSED, (u64)ex[s]); k12_add(o + SG_IMPACT_DIRECT, (u64)di[s]); k12_max(o + SG_IMPACT_FAR, far[s]);
        k12_add(o + SG_IMPACT_ENTRIES, (u64)en[s]); k12_add(o + SG_IMPACT_ENTRY_COUNT, ec[s]); k12_add(o + SG_IMPACT_ENTRY_ERR, ee[s]);
    }
}

__global__ __launch_bounds__(K12_THREADS) void k22_push(ImpactArgs a, u32 r) {
    if (a.cnt[r - 1] == 0) return;                                    // (uniform: round r - 1 gave no row a new bit)
    const u64 G = k16_edges_of(a.g);
    const u32 W = a.W;
    for (u64 j = (u64)blockIdx.x * K12_THREADS + threadIdx.x; j < G; j += (u64)gridDim.x * K12_THREADS) {
        const u64 e = a.ends[j];
        if (e == K22_NO_EDGE) continue;
        const u64 s = (u32)e, d = e >> 32;
        for (u32 w = 0; w < W; w++) {
            const u64 f = a.fresh[d * W + w];
            if (f) atomicOr(reinterpret_cast<unsigned long long*>(a.next + s * W + w), (unsigned long long)f);
        }
    }
}

__global__ __launch_bounds__(K12_THREADS) void k22_finish(ImpactArgs a) {
    const u32 cov = k22_covered(a);
    for (u64 i = (u64)blockIdx.x * K12_THREADS + threadIdx.x; i < cov; i += (u64)gridDim.x * K12_THREADS) {
        u64* f = a.out + i * SG_IMPACT_WORDS + SG_IMPACT_FAR;
        const u64 k = *f;
        *f = k ? (k & 0xFFFFFFFF00000000ull) | (u64)(~(u32)k) : 0x00000000FFFFFFFFull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.count = cov;
}
