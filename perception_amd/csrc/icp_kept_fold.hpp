// icp_kept_fold.hpp - the tail of the kernels that stand behind k_icp_iter<true>(it) in the sliced loop and REPLACE the iteration's
// slot with the sums of the correspondences an opt-in rule keeps (k_icp_reject, rule C19; k_icp_recip_fold, rule C22), written once:
// which clusters a launch leaves alone, one kept correspondence's moment_terms added to the lane's 64-bit sums (the fold over
// lanes and waves is common.hpp's wave_fold_to_lds), the plain vector stores of the slot's 16 sums, and the four fields every
// such rule reports (KeptStats, common.hpp).  One workgroup per cluster; integer sums, so nothing depends on which lane or wave
// took which point.  A kernel keeps what is its own: the predicate of its loop, its counts - one or two, which it folds and
// stores to d_ncorr itself - and the rest of its record.
#pragma once
#include "common.hpp"
#include "icp_solve.hpp"

namespace cd {

// a cluster the kernels of launch `it` leave alone: pre-marked, or finished (k_icp_solve(it) has run)
__device__ __forceinline__ bool kept_skips(const IcpCluster& c, const IcpState* __restrict__ st, int k, int it) {
    if (c.n < ICP_MIN_CORR || c.tpl_m <= 0) return true;
    return st[(size_t)k * 2 + (it & 1)].done || st[(size_t)k * 2 + ((it + 1) & 1)].done;
}

// point i of the cluster is kept: its terms join the lane's sums.  pts / nnp / tp: the cluster's points, their neighbours
// (positions k_icp_iter wrote; the clamp keeps a read inside the template of tpl_m points) and the template; d2 = the point's.
// (i by reference: it is the caller's loop counter, and a copy of it is one more variable for the compiler to order - the
// loop's instructions then come out in another order, and the two kernels were tuned in this one: profiles/EXPERIMENTS.md.)
__device__ __forceinline__ void kept_add(const float4* pts, const int* nnp, const float4* tp, int tpl_m, const int& i, float d2,
                                         unsigned long long (&S)[16]) {
    const float4 p = pts[i];
    const int j = min(max(nnp[i], 0), tpl_m - 1);
    const float4 q = tp[j];
    const float pv[3] = {p.x, p.y, p.z}, qv[3] = {q.x, q.y, q.z};
    unsigned long long t[16];
    moment_terms(pv, qv, d2, t);
#pragma unroll
    for (int a = 0; a < 16; ++a) S[a] += t[a];
}

// the slot of iteration `it`; threads 0 .. 15 store its sums (after the barrier that follows wave_fold_to_lds)
__device__ __forceinline__ size_t kept_store_sums(unsigned long long* acc, const unsigned long long* s_sum, int k, int it) {
    const int tid = threadIdx.x;
    const size_t slot = (size_t)k * 3 + (size_t)(it % 3);
    if (tid < 16) acc[slot * 16 + tid] = s_sum[tid];
    return slot;
}

// ONE thread, after it has stored the slot's count n to d_ncorr and read the cluster's record: the four fields of its head
__device__ __forceinline__ void kept_update(KeptStats& ks, int it, int n) {
    if (it == 0) { ks.first_kept = n; ks.min_kept = n; }
    else ks.min_kept = min(ks.min_kept, n);
    ks.last_kept = n;
    if (n < ICP_MIN_CORR) ks.stopped_few = 1;
}

}  // namespace cd
