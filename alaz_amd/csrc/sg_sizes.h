// sg_sizes.h — the kernels' fixed sizes that the host's sizing rules (sg_plan.hpp) also need.  No HIP: the planner includes
// it on the CPU, sg_device.h includes it for the kernels.
#pragma once

#define SG_MAX_K1_WGS 2048

// K1 pass A, 16-byte records (sg_k1_wide.h)
#define K1A_THREADS 1024
#define K1A_NJ      6         // 16-byte join-blob words a thread stages into LDS (6 * 1024 * 16 B = 96 KiB at most)
// K1 pass A, narrow records, one team per workgroup (sg_k1_narrow.h)
#define K1T_THREADS 1024
#define K1T_CHUNK   4096u         // events per chunk at most: four per thread
#define K1T_TS(NSUB) (K1T_CHUNK * (NSUB))   // records per tile: NSUB chunks (1 or 2)
// K1 pass A, two teams per workgroup (sg_k1_team.h)
// LDS besides the cache and the join tables: piece counters + per team 4 counter arrays, statistics + barrier words, tile(s) of 4 records per thread (+ trash words)
#define K1M_LDS_FIXED(np, teams, nt) ((size_t)(np) * 4 * (2 + 4 * (teams)) + 128 + ((size_t)(nt) * 4 + 4) * 8)
// ... and what the paired form (PAIR = 1) takes on top: a second tile's worth of records per team
#define K1M_LDS_PAIR_EXTRA(np, teams, nt) ((size_t)(nt) * 4 * 8)

// K2 (sg_k2.h)
#define K2_TILE 2048   // table slots per workgroup (256 threads x 8)
#define K2_DH_GMAX 128           // k2_rowptr keeps a row's column of counts in registers: GMAX / 8 per lane
#define K2_SORT_LDS 4096         // words of each of the row sort's two LDS arrays — at least: the host sizes them (Dev::k2_sortw) so that a node bitmap fits, up to K2_SORT_LDS_MAX
#define K2_SORT_LDS_MAX 16384

// K3 in-statistics (sg_k3.h)
#define K3_IN_NR    3072      // nodes per range: 3072 x 6 x 8 B = 144 KiB of LDS
#define K3_IN_SMAX  48        // edge slices at most (48 where ranges x 48 workgroups are one round of the chip, else 32: sg_plan.hpp)

// warm windows (sg_kw.h)
#define KW_ROWS 512                                                  // rows per chunk with LDS accumulators (5 x u64 each: 20 KiB)
