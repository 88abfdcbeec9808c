// sg_group_track.h — K19: each window's workload incidents followed across windows on the device (include/servicegraph.h,
// "workload tracks").  Included after sg_group_incident.h: K13's definition (sg_track.h) with "incident" read as "workload incident"
// (K18) and "node row" read as "workload row" (K16).
//
// Six of K13's eight kernels see the space only through the row count, the incident capacity and the ended capacity, all three
// TrkArgs.nd.ncap: k13_init, k13_fold, k13_claim, k13_count, k13_scan and k13_write are launched as they are, with nd.ncap = K16's
// nc and nodes / ncount / inc / icount / node_inc pointing at K16's and K18's slot buffers.  Only the anchor differs: a workload row
// anchors when its ref is a GROUP, KNOWN or LABEL ref, and its key is K16's group key (k16_gk(ref) < max_groups + mk + ml; an OBIP
// key lies above that bound, a ref beyond the id spaces has none).  So this file adds the space policy, k19_look over K13's body
// (k13_look_t: the wave reduction, the LDS table k12_slot / k12_add over K12_SLOTS and the fallback to device memory are K13's own
// code) and k19_members, k13_members' loop with the workload anchor.  The members are [max_groups + mk + ml] by that key; nothing
// migrates a member when sg_group_assign moves a pod between groups: the old key's member ages out after quiet_windows.
// Two plain launches among K13's six, no scratch memory.
#pragma once

static_assert(SG_NONE == K13_NONE, "k16_gk's 'no key' is k13's 'no anchor'");

struct K19Space {
    u32 max_groups;
    __device__ __forceinline__ u32 anchor(const TrkArgs& a, u32 ref) const {
        GroupNodesArgs g{};                                           // (k16_gk reads the id spaces and max_groups only)
        g.nd = a.nd; g.max_groups = max_groups;
        const u32 k = k16_gk(g, ref);                                 // (SG_NONE: no key, no anchor)
        return (u64)k < (u64)max_groups + a.nd.mk + a.nd.ml ? k : K13_NONE;
    }
};

__global__ __launch_bounds__(K13_THREADS) void k19_look(TrkArgs a, u32 max_groups) { k13_look_t(a, K19Space{max_groups}); }

__global__ __launch_bounds__(K13_THREADS) void k19_members(TrkArgs a, u32 max_groups) {
    const K19Space sp{max_groups};
    const u64 N = sg_nodes_of(a.ncount, a.nd.ncap);
    for (u64 v = (u64)blockIdx.x * K13_THREADS + threadIdx.x; v < N; v += (u64)gridDim.x * K13_THREADS) {
        const u32 i = a.node_inc[v];
        if (i == SG_NO_INCIDENT) continue;
        const u32 k = sp.anchor(a, a.nodes[v].ref);
        if (k == K13_NONE) continue;
        a.mtrack[k] = a.out[i].track; a.mlast[k] = a.w;
    }
}
