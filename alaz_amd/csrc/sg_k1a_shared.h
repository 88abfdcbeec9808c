// sg_k1a_shared.h — what the three pass-A kernels of K1 share: k1a_partition (sg_k1_wide.h), k1a_tile_partition (sg_k1_narrow.h) and
// k1a_team_partition (sg_k1_team.h).  Included by sg_kernels.h ahead of the three; in the order a kernel runs them: the join-blob
// staging, the two-level join, the cache accumulate, the workgroup's statistics line.  What is deliberately NOT here is what makes
// each kernel what it is: its event loads, its statistics policy, the P1-P4 tile structure and copy-outs of tile and team, team's
// batched level-1 loads, tickets, team barriers and kd().
#pragma once

// Issue a global load NOW and leave it in flight; a later s_waitcnt (inline asm that names the
// destination registers as in/out operands) is the matching wait.  Written as inline asm because the
// compiler puts waits between conditional loads.  vmcnt is in-order for loads, so the compiler's own
// (unaware) waits can only become stronger, never too weak.  Rule: no loop-carried value and no branch
// merge between an issue and its wait (a compiler-inserted register copy there would read a register that
// is still being loaded).
typedef u32 v4u_t __attribute__((ext_vector_type(4)));
typedef u32 v2u_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gload16_issue(v4u_t& dst, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(dst) : "v"(p) : "memory"); }

// exact for every 32-bit duration: floor(x / 1000) = (x * 0x10624DD3) >> 38
__device__ __forceinline__ u32 div1000_u32(u32 x) { return __umulhi(x, 0x10624DD3u) >> 6; }

// ---- the join blob -> LDS ---------------------------------------------------------------------------------------------------
// The blob is d.jstage_bytes >> 4 16-byte words: level 1 (always there), then level 2 when it is staged.  Thread t of NT takes
// words t + k NT, k < K1A_NJ.  Source address of the k-th (a lane beyond the blob re-reads its last word and does not store it):
template <int NT>
__device__ __forceinline__ const uint4* k1a_join_src(const Dev& d, u32 t, u32 k) {
    const u32 n16 = d.jstage_bytes >> 4, n1 = (d.jl1mask + 1) >> 1;   // 16-byte words to stage; of them level 1
    const u32 i = t + k * NT < n16 ? t + k * NT : n16 - 1;
    return (i < n1 ? reinterpret_cast<const uint4*>(d.jl1) : reinterpret_cast<const uint4*>(d.jl2) - n1) + i;
}
// ... and its store: level-1 words go in as they are; with L2M == 2 a level-2 word = four u32 entries kind << 30 | id becomes four
// u16 entries kind << 14 | id
template <int NT, int L2M>
__device__ __forceinline__ void k1a_join_store(const Dev& d, uint4* jl, u32 t, u32 k, const v4u_t r) {
    const u32 n16 = d.jstage_bytes >> 4, n1 = (d.jl1mask + 1) >> 1, i = t + k * NT;
    auto p16 = [](u32 x) { return ((x >> 30) << 14) | (x & 0x3FFFu); };
    if (i < n16) {
        if (L2M == 2 && i >= n1) reinterpret_cast<uint2*>(jl + n1)[i - n1] = make_uint2(p16(r.x) | (p16(r.y) << 16), p16(r.z) | (p16(r.w) << 16));
        else jl[i] = make_uint4(r.x, r.y, r.z, r.w);
    }
}
// Six 16-byte loads per lane at most, issued and waited for in ONE asm statement: between a hand-issued load and the wait that
// names its registers there must be no code at all (a loop there once made the register allocator move in-flight registers: the
// staged join table came out as garbage -> wild record addresses -> a memory fault, or a few hundred silently lost events).  For
// the same reason the caller's LDS set-up (ordinary loads and stores) comes BEFORE this call.
template <int NT, int L2M>
__device__ __forceinline__ void k1a_stage_join(const Dev& d, uint4* jl, u32 t) {
    static_assert(K1A_NJ == 6, "written out for 6 blob words per lane");
    v4u_t jb0, jb1, jb2, jb3, jb4, jb5;
    const uint4* js0 = k1a_join_src<NT>(d, t, 0); const uint4* js1 = k1a_join_src<NT>(d, t, 1); const uint4* js2 = k1a_join_src<NT>(d, t, 2);
    const uint4* js3 = k1a_join_src<NT>(d, t, 3); const uint4* js4 = k1a_join_src<NT>(d, t, 4); const uint4* js5 = k1a_join_src<NT>(d, t, 5);
    asm volatile("global_load_dwordx4 %0, %6, off\n\tglobal_load_dwordx4 %1, %7, off\n\tglobal_load_dwordx4 %2, %8, off\n\t"
                 "global_load_dwordx4 %3, %9, off\n\tglobal_load_dwordx4 %4, %10, off\n\tglobal_load_dwordx4 %5, %11, off\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(jb0), "=&v"(jb1), "=&v"(jb2), "=&v"(jb3), "=&v"(jb4), "=&v"(jb5)
                 : "v"(js0), "v"(js1), "v"(js2), "v"(js3), "v"(js4), "v"(js5) : "memory");
    k1a_join_store<NT, L2M>(d, jl, t, 0, jb0); k1a_join_store<NT, L2M>(d, jl, t, 1, jb1); k1a_join_store<NT, L2M>(d, jl, t, 2, jb2);
    k1a_join_store<NT, L2M>(d, jl, t, 3, jb3); k1a_join_store<NT, L2M>(d, jl, t, 4, jb4); k1a_join_store<NT, L2M>(d, jl, t, 5, jb5);
}

// ---- the fast path's join: two-level block table, level 1 in LDS, branch-free ---------------------------------------------
// L2M: level 2 is read through l2 (u32 entries kind << 30 | id; LDS or global memory) or, L2M == 2, l2h (u16 entries kind << 14 | id)
template <int L2M>
__device__ __forceinline__ u32 k1a_join(const u64* l1, const u32* l2, const unsigned short* l2h, u32 jl1mask, u32 ip) {
    const u32 b = ip >> 8;
    const u64 e1 = l1[((__umul24(b, SG_JL1_K1)) >> 9) & jl1mask], e2 = l1[((__umul24(b, SG_JL1_K2)) >> 11) & jl1mask];
    const u32 blk = (u32)e1 == b ? (u32)(e1 >> 32) : ((u32)e2 == b ? (u32)(e2 >> 32) : 0u);     // block 0 = the all-zero block
    return L2M == 2 ? (u32)l2h[(blk << 8) | (ip & 255u)] : l2[(blk << 8) | (ip & 255u)];
}

// ---- the fast-path decision (data.go:827-870, dto.go:226-231 as selects) is NOT shared: one function for it, called by the three
// kernels, computed the same values but moved every kernel's register allocation — k1a_partition 95 -> 97 VGPRs, k1a_team_partition
// by 1 to 4 VGPRs either way with scratch 28 -> 20 and 12 -> 0 bytes in three instantiations, k1a_tile_partition with two sub-tiles
// +220 to +310 instructions and scratch 80 -> 84 — whether it returned a struct or wrote references, in whatever order it was written.
// The three copies stay (K1A_FAST, tile's `fast`, team's `front2`) and point at one another.  The cache flush at the end of tile and team
// (the same eleven lines) also stays where it is: as one function it cost three k1a_tile_partition instantiations a spilled SGPR each.

// ---- cache accumulate of one accepted event into a slot its key owns: count | err << 32, sum, max, sum of squared microseconds
// DUR32: the caller knows dur < 2^32 at compile time (us < 2^23: 24-bit multiplies); otherwise the 64-bit divide is the rare arm
template <bool DUR32>
__device__ __forceinline__ void k1a_cache_add(u64* cacc, u32 slot, u64 dur, u32 err) {
    u64 ssq;
    if (DUR32 || (dur >> 32) == 0) { const u32 us = div1000_u32((u32)dur); ssq = (u64)us * (u64)us; }
    else { const u64 us = dur / 1000ull; ssq = us * us; }
    atomicAdd(&cacc[slot * 4], 1ull | ((u64)err << 32)); atomicAdd(&cacc[slot * 4 + 1], dur);
    atomicMax(&cacc[slot * 4 + 2], dur); atomicAdd(&cacc[slot * 4 + 3], ssq);
}

// ---- the workgroup's statistics line -------------------------------------------------------------------------------------------
// red: [8] u64 in LDS, WS_* order (WS_PAD = accepted, then dropped for capacity); a K1Local is added to it where it was filled
__device__ __forceinline__ void k1_red_add(u64* red, const K1Local& x) {
    if (x.acc) { atomicAdd(&red[WS_ACCEPTED], (u64)x.acc); atomicMin(&red[WS_TMIN], x.tmin); atomicMax(&red[WS_TMAX], x.tmax); }
    if (x.lost) atomicAdd(&red[WS_PAD], (u64)x.lost);
    if (x.maxlabel) atomicMax(&red[WS_MAXLABEL], (u64)x.maxlabel);
    if (x.dsrc) atomicAdd(&red[WS_DROPPED_SRC], (u64)x.dsrc);
    if (x.dcap) atomicAdd(&red[WS_DROPPED_CAP], (u64)x.dcap);
    if (x.misr) atomicAdd(&red[WS_MISROUTED], (u64)x.misr);
}
// the end of the kernel (one thread, behind a barrier): red -> this workgroup's private 64-byte line of d.wgstat
__device__ __forceinline__ void k1_publish_wg(const Dev& d, const u64* red) {
    u64* g = d.wgstat + (size_t)(blockIdx.x % SG_MAX_K1_WGS) * WS_WORDS;
    // accepted = counted by the lanes - dropped afterwards for capacity (a workgroup only drops what it accepted itself)
    if (red[WS_ACCEPTED]) { atomicMin(&g[WS_TMIN], red[WS_TMIN]); atomicMax(&g[WS_TMAX], red[WS_TMAX]); atomicAdd(&g[WS_ACCEPTED], red[WS_ACCEPTED] - red[WS_PAD]); }
    if (red[WS_MAXLABEL]) atomicMax(&g[WS_MAXLABEL], red[WS_MAXLABEL]);
    if (red[WS_DROPPED_SRC]) atomicAdd(&g[WS_DROPPED_SRC], red[WS_DROPPED_SRC]);
    if (red[WS_DROPPED_CAP]) atomicAdd(&g[WS_DROPPED_CAP], red[WS_DROPPED_CAP]);
    if (red[WS_MISROUTED]) atomicAdd(&g[WS_MISROUTED], red[WS_MISROUTED]);
}
