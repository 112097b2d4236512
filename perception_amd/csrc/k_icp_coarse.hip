// k_icp_coarse.hip - the two device steps of canonical rule C18 (perception_amd/icp_coarse.py is the
// specification) around the ICP drivers, which run both levels as they stand:
//   k_icp_coarse_gather     before the coarse stage: every eligible problem's strided subsample, packed into the coarse region of
//                           the source buffers (both copies: the drivers move d_src in place and keep d_src0)
//   k_icp_coarse_handover   inside the fine stage's set-up, after its states are up: per fine problem the decision of step 4 on
//                           the coarse state, T_c (or the call's own guess) into the guess slot that k_icp_apply_guess reads and
//                           into Tfinal of both parity states, and the pair's stats record
// No atomics, no LDS; the tables come from plan_coarse (icp_coarse_plan.hpp).
#include "kernels.hpp"
#include "icp_coarse_plan.hpp"

namespace cd {

// One workgroup row per coarse problem (blockIdx.x), blockIdx.y strides over its points: the reads are `stride` records apart, the
// writes of a wave are consecutive 16-byte records.  pts0 is read (the clusters) and written (the coarse region behind them).
__global__ void __launch_bounds__(BLOCK) k_icp_coarse_gather(const CoarseGather* __restrict__ tab, float4* pts0, float4* __restrict__ pts) {
    const CoarseGather g = tab[blockIdx.x];
    for (int j = blockIdx.y * BLOCK + threadIdx.x; j < g.n_coarse; j += gridDim.y * BLOCK) {
        const float4 p = pts0[(size_t)g.src_off + (size_t)j * (size_t)g.stride];
        pts0[(size_t)g.dst_off + j] = p;
        pts[(size_t)g.dst_off + j] = p;
    }
}

// One lane per fine problem.  cst[j] / caccf[j]: the final state (parity slot 0) and fitness sum of coarse problem j.
__global__ void __launch_bounds__(WAVE) k_icp_coarse_handover(int ncl, const CoarseHand* __restrict__ hand, const IcpState* __restrict__ cst,
                                                              const unsigned long long* __restrict__ caccf, IcpState* __restrict__ st,
                                                              float* __restrict__ guess, CoarseStats* __restrict__ stats) {
    const int k = blockIdx.x * WAVE + threadIdx.x;
    if (k >= ncl) return;
    const CoarseHand h = hand[k];
    CoarseStats s;
    s.n_coarse = 0; s.coarse_iterations = 0; s.coarse_converged = 0; s.coarse_status = CD_OK; s.coarse_fitness = 0.0;
    s.used = COARSE_NOT_ELIGIBLE; s.reserved = 0;
    if (h.coarse >= 0) {
        const IcpState cs = cst[h.coarse];
        int fall_back = 0;
        s.coarse_status = coarse_handover(cs.status, cs.converged, cs.Tfinal, &fall_back);
        s.n_coarse = h.n_coarse;
        s.coarse_iterations = cs.iters;
        s.coarse_converged = cs.converged;
        // (fill_cluster_result's expression)
        s.coarse_fitness = cs.status == CD_OK ? ldexp((double)(long long)caccf[h.coarse], -FIX_SHIFT_D2) / (double)h.n_coarse : 1.7976931348623157e308;
        s.used = fall_back ? COARSE_FELL_BACK : COARSE_USED;
        if (!fall_back)
            for (int i = 0; i < 16; ++i) { st[2 * (size_t)k].Tfinal[i] = cs.Tfinal[i]; st[2 * (size_t)k + 1].Tfinal[i] = cs.Tfinal[i]; }
    }
    // the guess the sources are moved by: T_c, or what the stage's own set-up left in Tfinal (identity, the call's guess, rule C13's)
    for (int i = 0; i < 16; ++i) guess[16 * (size_t)k + i] = st[2 * (size_t)k].Tfinal[i];
    stats[k] = s;
}

void launch_icp_coarse_gather(hipStream_t s, int n_coarse_problems, int max_n_coarse, const CoarseGather* tab, float4* src0, float4* src) {
    if (n_coarse_problems <= 0 || max_n_coarse <= 0) return;
    const int gy = (max_n_coarse + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_icp_coarse_gather, dim3(n_coarse_problems, gy < 64 ? gy : 64), dim3(BLOCK), 0, s, tab, src0, src);
}

void launch_icp_coarse_handover(hipStream_t s, int ncl, const CoarseHand* hand, const IcpState* cst, const unsigned long long* caccf, IcpState* st,
                                float* guess, CoarseStats* stats) {
    if (ncl <= 0) return;
    hipLaunchKernelGGL(k_icp_coarse_handover, dim3((ncl + WAVE - 1) / WAVE), dim3(WAVE), 0, s, ncl, hand, cst, caccf, st, guess, stats);
}

}  // namespace cd
