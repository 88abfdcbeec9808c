// sg_track.h — K13: each window's incidents followed across windows on the device (include/servicegraph.h, "tracks").
// Included after sg_incident.h: it reads K12's incident rows and the incident per node row, reuses K9's node key (k9_node) and K12's
// LDS fold (k12_slot / k12_add), and adds kernels of its own.
//
// Kept state: the members, two u32 arrays (track, last) indexed by the anchor's node key (k9_node(ref) < mk + ml: KNOWN and LABEL
// refs; an OBIP key is an index into one window's list and carries no membership), and the track table, sorted by id, double
// buffered, looked up by binary search, with its counters (TrkState) double buffered beside it: a launch reads one copy and the
// scan's thread 0 writes the other, so no workgroup reads a word another one of the same launch writes.  Nothing is zeroed between
// windows: the passes rewrite every per-incident, per-node-row and per-entry word they read.  Every field is an integer sum, an
// integer max, a min of ids or the max of a (kept << 32 | ~incident) key: one value whatever order lanes and workgroups run in.
// Eight plain launches on the window's stream behind K12; no workgroup ever waits for another.
//
//   k13_init     per incident: cand = SG_NO_TRACK, kept = moved = joined = 0; per table entry: its claim word = 0
//   k13_look     per node row in an incident: an anchor?  t_v = its live member's track (the member young enough and its id in
//                the table), kept per node row for the next pass; cand (min) and joined folded per incident
//   k13_fold     per node row with a t_v: kept (t_v == cand) or moved, folded per incident
//   k13_claim    per incident with a cand: the candidate's table position; the claim: one 64-bit max of kept << 32 | ~incident
//   k13_count    per workgroup span of incidents and table entries: the opened tracks, the kept entries, the ended entries
//   k13_scan     (1 workgroup) exclusive scans of the three counts; the next state: entries, next_id, the totals; the ended count
//   k13_write    the incident's sg_incident_track row; the kept entries (a continued one updated) compacted into the other table
//                buffer, the opened ones appended in incident order, both below max_tracks; the ended list
//   k13_members  per anchor in an incident: member = (the incident's track, w)
//
// k13_look and k13_fold fold as k12_nodes does: a wave whose active lanes name one incident reduces in registers, every
// contribution then goes to an LDS table keyed by incident, and a workgroup touches device memory once per field and distinct
// incident; only an incident that finds no slot is folded into device memory directly.
//
// Six of the eight see the space only through the row count and the capacities (nd.ncap); k13_look and k13_members also ask which
// rows anchor.  k13_look's body is a template over a space policy (k13_look_t): sp.anchor(a, ref) is the anchor key of a row's ref,
// K13_NONE for a row that is no anchor.  K13Space below is this stage's; K19's is in sg_group_track.h, beside its own k19_members
// (k13_members as a template did not compile to the same code, so it stays as it was, written out).
#pragma once

#define K13_THREADS 256
#define K13_MAX_WGS 1024          // workgroups of k13_count / k13_write at most (k13_scan scans one count per thread)
#define K13_SCAN_THREADS 1024
#define K13_BLK_WORDS (7 * K13_MAX_WGS)   // three count arrays, their three scans, the three totals
#define K13_NONE 0xFFFFFFFFu

static_assert(sizeof(sg_incident_track) == 32 && sizeof(sg_track_entry) == 40 && offsetof(sg_track_entry, count) == 24 &&
              sizeof(sg_track_params) == 16 && sizeof(sg_track_stats) == 32, "sg_incident_track / sg_track_entry / sg_track_params layout");

// the table's counters; one copy is read and the other written per window
struct TrkState { u32 n, next_id; u64 opened, dropped; };

struct TrkArgs {
    NodesArgs nd;                 // K9's part: mk, ml, mob, ncap (k9_node)
    const sg_node_out* nodes;     // the window's node rows
    const u64* ncount;            // their count
    const sg_incident_out* inc;   // the window's incidents (K12)
    const u64* icount;            // their count
    const u32* node_inc;          // the incident per node row
    u32 w, quiet, max_tracks;
    u32 per;                      // incidents / entries per workgroup of k13_count / k13_write (a multiple of K13_THREADS)
    u32* mtrack; u32* mlast;      // [mk + ml] the members by anchor key
    const sg_track_entry* told; sg_track_entry* tnew;   // [max_tracks] the table before and after this window
    const TrkState* sold; TrkState* snew;
    u32* cand; u32* kept; u32* moved; u32* joined; u32* pos;   // [ncap] by incident
    u32* tv;                      // [ncap] by node row
    u64* claim;                   // [max_tracks] by table position
    u32* blk;                     // [K13_BLK_WORDS]
    sg_incident_track* out;       // [ncap] this window's rows
    sg_track_entry* ended;        // [ncap] this window's ended list
    u64* ended_count;
};

__device__ __forceinline__ u32 k13_incidents_of(const TrkArgs& a) { const u64 I = *a.icount; return (u32)(I < a.nd.ncap ? I : (u64)a.nd.ncap); }
__device__ __forceinline__ u32 k13_entries_of(const TrkArgs& a) { const u32 n = a.sold->n; return n < a.max_tracks ? n : a.max_tracks; }
// the anchor key of a node row's ref, K13_NONE for an OBIP ref (and a ref beyond the id spaces)
__device__ __forceinline__ u32 k13_anchor(const TrkArgs& a, u32 ref) { const u32 k = k9_node(a.nd, ref); return k < a.nd.mk + a.nd.ml ? k : K13_NONE; }
// K13's space: K9's node keys
struct K13Space {
    __device__ __forceinline__ u32 anchor(const TrkArgs& a, u32 ref) const { return k13_anchor(a, ref); }
};
// the table position of track id, K13_NONE when the table lacks it
__device__ __forceinline__ u32 k13_find(const sg_track_entry* t, u32 n, u32 id) {
    u32 lo = 0, hi = n;
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (t[m].track < id) lo = m + 1; else hi = m; }
    return (lo < n && t[lo].track == id) ? lo : K13_NONE;
}
// p may point to LDS or to device memory; SG_NO_TRACK is "nothing"
__device__ __forceinline__ void k13_min(u32* p, u32 x) { if (x != SG_NO_TRACK) atomicMin(p, x); }

__global__ __launch_bounds__(K13_THREADS) void k13_init(TrkArgs a) {
    const u32 I = k13_incidents_of(a), n = k13_entries_of(a), top = I > n ? I : n;
    for (u64 x = (u64)blockIdx.x * K13_THREADS + threadIdx.x; x < top; x += (u64)gridDim.x * K13_THREADS) {
        if (x < I) { a.cand[x] = SG_NO_TRACK; a.kept[x] = 0; a.moved[x] = 0; a.joined[x] = 0; }
        if (x < n) a.claim[x] = 0;
    }
}

template <class S>
__device__ __forceinline__ void k13_look_t(TrkArgs a, S sp) {
    __shared__ u32 key[K12_SLOTS], mn[K12_SLOTS], jn[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K13_THREADS) { key[s] = K12_EMPTY; mn[s] = SG_NO_TRACK; jn[s] = 0; }
    __syncthreads();
    const u32 n = k13_entries_of(a);
    const u64 N = sg_nodes_of(a.ncount, a.nd.ncap), stride = (u64)gridDim.x * K13_THREADS;
    for (u64 vb = (u64)blockIdx.x * K13_THREADS; vb < N; vb += stride) {   // (uniform per wave: the wave reductions see 64 lanes)
        const u64 v = vb + t;
        u32 i = SG_NO_INCIDENT, tv = SG_NO_TRACK;
        if (v < N) {
            const u32 ii = a.node_inc[v];
            const u32 k = ii != SG_NO_INCIDENT ? sp.anchor(a, a.nodes[v].ref) : K13_NONE;
            if (k != K13_NONE) {
                i = ii;
                const u32 T = a.mtrack[k];
                if (T != SG_NO_TRACK && a.w - a.mlast[k] - 1 <= a.quiet && k13_find(a.told, n, T) != K13_NONE) tv = T;
            }
            a.tv[v] = tv;
        }
        const bool act = i != SG_NO_INCIDENT;
        const u64 m = __ballot(act);
        if (!m) continue;
        const u32 lead = (u32)(__ffsll((long long)m) - 1);
        const u32 i0 = __shfl(i, lead, 64);
        const bool one = __ballot(act && i != i0) == 0;              // every active lane names one incident
        u32 c = tv, j = (act && tv == SG_NO_TRACK) ? 1u : 0u;         // (an inactive lane: SG_NO_TRACK and 0, nothing)
        if (one) { c = wave_min_u32(c); j = wave_sum_u32(j); }
        if (one ? (t & 63) == lead : act) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k13_min(&mn[s], c); k12_add(&jn[s], j); }
            else { k13_min(&a.cand[i], c); k12_add(&a.joined[i], j); }
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K13_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        k13_min(&a.cand[i], mn[s]); k12_add(&a.joined[i], jn[s]);
    }
}

__global__ __launch_bounds__(K13_THREADS) void k13_look(TrkArgs a) { k13_look_t(a, K13Space{}); }

__global__ __launch_bounds__(K13_THREADS) void k13_fold(TrkArgs a) {
    __shared__ u32 key[K12_SLOTS], kp[K12_SLOTS], mv[K12_SLOTS];
    const u32 t = threadIdx.x;
    for (u32 s = t; s < K12_SLOTS; s += K13_THREADS) { key[s] = K12_EMPTY; kp[s] = 0; mv[s] = 0; }
    __syncthreads();
    const u64 N = sg_nodes_of(a.ncount, a.nd.ncap), stride = (u64)gridDim.x * K13_THREADS;
    for (u64 vb = (u64)blockIdx.x * K13_THREADS; vb < N; vb += stride) {   // (uniform per wave)
        const u64 v = vb + t;
        u32 i = SG_NO_INCIDENT, k = 0, x = 0;
        if (v < N) {
            const u32 tv = a.tv[v];
            if (tv != SG_NO_TRACK) {                                  // (k13_look gave it one: the row is an anchor in an incident)
                i = a.node_inc[v];
                if (tv == a.cand[i]) k = 1; else x = 1;
            }
        }
        const bool act = i != SG_NO_INCIDENT;
        const u64 m = __ballot(act);
        if (!m) continue;
        const u32 lead = (u32)(__ffsll((long long)m) - 1);
        const u32 i0 = __shfl(i, lead, 64);
        const bool one = __ballot(act && i != i0) == 0;
        if (one) { k = wave_sum_u32(k); x = wave_sum_u32(x); }
        if (one ? (t & 63) == lead : act) {
            const u32 s = k12_slot(key, i);
            if (s != K12_EMPTY) { k12_add(&kp[s], k); k12_add(&mv[s], x); }
            else { k12_add(&a.kept[i], k); k12_add(&a.moved[i], x); }
        }
    }
    __syncthreads();
    for (u32 s = t; s < K12_SLOTS; s += K13_THREADS) {
        const u32 i = key[s];
        if (i == K12_EMPTY) continue;
        k12_add(&a.kept[i], kp[s]); k12_add(&a.moved[i], mv[s]);
    }
}

__global__ __launch_bounds__(K13_THREADS) void k13_claim(TrkArgs a) {
    const u32 I = k13_incidents_of(a), n = k13_entries_of(a);
    for (u64 i = (u64)blockIdx.x * K13_THREADS + threadIdx.x; i < I; i += (u64)gridDim.x * K13_THREADS) {
        const u32 c = a.cand[i];
        if (c == SG_NO_TRACK) continue;
        const u32 p = k13_find(a.told, n, c);                         // (k13_look found it in this table)
        a.pos[i] = p;
        if (p != K13_NONE) atomicMax(&a.claim[p], ((u64)a.kept[i] << 32) | (u64)(~(u32)i));   // (kept >= 1: never 0)
    }
}

// does incident i continue its candidate (is it the claimant)?
__device__ __forceinline__ bool k13_continues(const TrkArgs& a, u32 i) {
    if (a.cand[i] == SG_NO_TRACK) return false;
    const u32 p = a.pos[i];
    return p != K13_NONE && ~(u32)a.claim[p] == i;
}
// entry e, not continued at window w: does it stay in the table, and is this its first silent window?
__device__ __forceinline__ bool k13_stays(const TrkArgs& a, const sg_track_entry& e) { return a.w - e.last_window <= a.quiet; }
__device__ __forceinline__ bool k13_ends(const TrkArgs& a, const sg_track_entry& e) { return e.last_window + 1 == a.w; }

__global__ __launch_bounds__(K13_THREADS) void k13_count(TrkArgs a) {
    __shared__ u32 ws[3][K13_THREADS / 64];
    const u32 t = threadIdx.x, I = k13_incidents_of(a), n = k13_entries_of(a), top = I > n ? I : n;
    const u64 x0 = (u64)blockIdx.x * a.per, x1 = x0 + a.per < top ? x0 + a.per : top;
    u32 co = 0, ck = 0, ce = 0;
    for (u64 x = x0 + t; x < x1; x += K13_THREADS) {
        if (x < I) co += k13_continues(a, (u32)x) ? 0u : 1u;
        if (x < n) {
            const sg_track_entry e = a.told[x];
            const bool cont = a.claim[x] != 0;
            ck += (cont || k13_stays(a, e)) ? 1u : 0u;
            ce += (!cont && k13_ends(a, e)) ? 1u : 0u;
        }
    }
    co = wave_sum_u32(co); ck = wave_sum_u32(ck); ce = wave_sum_u32(ce);
    if ((t & 63) == 0) { ws[0][t >> 6] = co; ws[1][t >> 6] = ck; ws[2][t >> 6] = ce; }
    __syncthreads();
    if (t < 3) {
        u32 s = 0;
        for (int w = 0; w < K13_THREADS / 64; w++) s += ws[t][w];
        a.blk[t * K13_MAX_WGS + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(K13_SCAN_THREADS) void k13_scan(TrkArgs a, u32 nwg) {
    __shared__ u32 wsum[K13_SCAN_THREADS / 64 + 1];
    const u32 t = threadIdx.x;
    u32 tot[3];
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const u32 c = t < nwg ? a.blk[f * K13_MAX_WGS + t] : 0u;
        const u32 x = block_excl_scan<K13_SCAN_THREADS>(c, wsum, &tot[f]);
        if (t < nwg) a.blk[(3 + f) * K13_MAX_WGS + t] = x;
    }
    if (t == 0) {
        const TrkState o = *a.sold;
        const u64 all = (u64)tot[0] + tot[1];
        TrkState s;
        s.n = (u32)(all < a.max_tracks ? all : (u64)a.max_tracks);
        s.next_id = o.next_id + tot[0];
        s.opened = o.opened + tot[0];
        s.dropped = o.dropped + (all - s.n);
        *a.snew = s;
        *a.ended_count = tot[2];
        a.blk[6 * K13_MAX_WGS] = tot[0]; a.blk[6 * K13_MAX_WGS + 1] = tot[1]; a.blk[6 * K13_MAX_WGS + 2] = tot[2];
    }
}

__global__ __launch_bounds__(K13_THREADS) void k13_write(TrkArgs a) {
    __shared__ u32 wsum[K13_THREADS / 64 + 1];
    const u32 t = threadIdx.x, I = k13_incidents_of(a), n = k13_entries_of(a), top = I > n ? I : n;
    const u64 x0 = (u64)blockIdx.x * a.per, x1 = x0 + a.per < top ? x0 + a.per : top;
    u32 bo = a.blk[3 * K13_MAX_WGS + blockIdx.x], bk = a.blk[4 * K13_MAX_WGS + blockIdx.x], be = a.blk[5 * K13_MAX_WGS + blockIdx.x];
    const u32 kept_all = a.blk[6 * K13_MAX_WGS + 1], next_id = a.sold->next_id;
    for (u64 xb = x0; xb < x1; xb += K13_THREADS) {                 // (uniform: every thread takes every round)
        const u64 x = xb + t;
        // the incident's row; an opened track's entry
        const bool isi = x < x1 && x < I;
        const bool cont = isi && k13_continues(a, (u32)x);
        u32 tot;
        const u32 xo = block_excl_scan<K13_THREADS>((isi && !cont) ? 1u : 0u, wsum, &tot);
        if (isi) {
            const u32 c = a.cand[x], mv = a.moved[x];
            sg_incident_track r;
            r.kept_nodes = a.kept[x]; r.moved_nodes = mv; r.joined_nodes = a.joined[x];
            r.flags = mv ? SG_TRACK_MERGED : 0u;
            if (cont) {
                const sg_track_entry e = a.told[a.pos[x]];
                r.track = c; r.parent = e.parent; r.first_window = e.first_window; r.windows = e.windows + 1;
            } else {
                const u32 rank = bo + xo;
                r.track = next_id + rank; r.parent = c; r.first_window = a.w; r.windows = 1;
                r.flags |= SG_TRACK_NEW | (c != SG_NO_TRACK ? SG_TRACK_SPLIT : 0u);
                const u64 at = (u64)kept_all + rank;
                if (at < a.max_tracks) {
                    const sg_incident_out* o = a.inc + x;
                    sg_track_entry e;
                    e.track = r.track; e.parent = c; e.first_window = a.w; e.last_window = a.w; e.windows = 1; e.peak_nodes = o->nodes;
                    e.count = o->count; e.err = o->err;
                    a.tnew[at] = e;
                }
            }
            a.out[x] = r;
        }
        bo += tot;
        // the table entry: kept (a continued one updated), ended, or forgotten
        const bool ise = x < x1 && x < n;
        sg_track_entry e{};
        u64 cl = 0;
        if (ise) { e = a.told[x]; cl = a.claim[x]; }
        const bool keep = ise && (cl != 0 || k13_stays(a, e)), end = ise && cl == 0 && k13_ends(a, e);
        const u32 xk = block_excl_scan<K13_THREADS>(keep ? 1u : 0u, wsum, &tot);
        u32 tote;
        const u32 xe = block_excl_scan<K13_THREADS>(end ? 1u : 0u, wsum, &tote);
        if (end && be + xe < a.nd.ncap) a.ended[be + xe] = e;        // (as it stood; at most one window's incidents end at once)
        if (keep && bk + xk < a.max_tracks) {
            if (cl != 0) {
                const sg_incident_out* o = a.inc + (~(u32)cl);
                e.last_window = a.w; e.windows += 1; e.peak_nodes = e.peak_nodes > o->nodes ? e.peak_nodes : o->nodes;
                e.count += o->count; e.err += o->err;
            }
            a.tnew[bk + xk] = e;
        }
        bk += tot; be += tote;
    }
}

__global__ __launch_bounds__(K13_THREADS) void k13_members(TrkArgs a) {
    const u64 N = sg_nodes_of(a.ncount, a.nd.ncap);
    for (u64 v = (u64)blockIdx.x * K13_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K13_THREADS) {
        const u32 i = a.node_inc[v];
        if (i == SG_NO_INCIDENT) continue;
        const u32 k = k13_anchor(a, a.nodes[v].ref);
        if (k == K13_NONE) continue;
        a.mtrack[k] = a.out[i].track; a.mlast[k] = a.w;
    }
}
