// icp_debug.hpp - the ICP kernels' instrumentation (experiment builds only: tools/README.md).  A device global belongs to one
// unit: k_icp_pipe.hip owns the counters of k_icp_pipe / k_icp_pipe_big (-DCD_STATS, -DCD_TIMERS [-DCD_TIMERS_FETCH],
// -DCD_ITSTATS, -DCD_DONDBG), k_icp.hip those of k_icp_persist (-DCD_PERSISTDBG).  Without a switch every macro here is empty.
#pragma once
#include "common.hpp"

// A counter array and its getter: copies the array out and, if `reset`, zeroes it.  dims: [16], [32][4], ...
#define CD_DEBUG_COUNTERS(var, dims, getter)                                                                  \
    __device__ unsigned long long var dims;                                                                   \
    extern "C" int getter(unsigned long long* out, int reset) {                                               \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(var), sizeof(var)) != hipSuccess) return -1;                  \
        if (reset) { static const unsigned long long z dims = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(var), z, sizeof(z)); } \
        return 0;                                                                                             \
    }

// cycles since the last mark go to phase n of the enclosing kernel's tph[]; at its end: into g_icp_stats[8 + n], and the workgroup's busy time (100 MHz wall clock) into [14] sum, [15] max, [7] count
#ifdef CD_TIMERS
#define CD_TIMERS_BEGIN long long tph[6] = {0, 0, 0, 0, 0, 0}, tlast = clock64(); const long long wg_t0_ = wall_clock64();
#define CD_PHASE(n) { const long long tn_ = clock64(); tph[n] += tn_ - tlast; tlast = tn_; }
#define CD_TIMERS_END { if ((threadIdx.x & 63) == 0) for (int i = 0; i < 6; ++i) atomicAdd(&g_icp_stats[8 + i], (unsigned long long)tph[i]); \
    if (threadIdx.x == 0) { const unsigned long long dt = (unsigned long long)(wall_clock64() - wg_t0_); \
                            atomicAdd(&g_icp_stats[14], dt); atomicMax(&g_icp_stats[15], dt); atomicAdd(&g_icp_stats[7], 1ull); } }
#else
#define CD_TIMERS_BEGIN
#define CD_PHASE(n)
#define CD_TIMERS_END
#endif

// one event in quarter-millisecond bin b of the workgroup's own life (100 MHz ticks since t0): g_don_dbg[slot0 + b]; DON_DBG_WAIT_*: around a wait for a handed-over cluster
#ifdef CD_DONDBG
#define DON_DBG(slot0, t0) atomicAdd(&g_don_dbg[(slot0) + min(15, (int)((wall_clock64() - (t0)) / 25000))], 1ull)
#define DON_DBG_BEGIN const long long don_t0 = wall_clock64();
#define DON_DBG_WAIT_BEGIN DON_DBG(8, don_t0); const long long tw0_ = wall_clock64();
#define DON_DBG_WAIT_END(k) { atomicAdd(&g_don_dbg[2], (unsigned long long)(wall_clock64() - tw0_)); \
    if ((k) >= 0) DON_DBG(40, don_t0); else atomicMax(&g_don_dbg[1], (unsigned long long)(wall_clock64() - don_t0)); }
#else
#define DON_DBG(slot0, t0)
#define DON_DBG_BEGIN
#define DON_DBG_WAIT_BEGIN
#define DON_DBG_WAIT_END(k)
#endif

// workgroup 0's ticks since the last mark go to g_persist_dbg[k]
#ifdef CD_PERSISTDBG
#define PERSIST_PHASE(k) { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); g_persist_dbg[k] += t_ - tdbg_; tdbg_ = t_; } }
#else
#define PERSIST_PHASE(k)
#endif
