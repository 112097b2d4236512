// icp_coarse_plan.hpp - the host arithmetic of canonical rule C18 (perception_amd/icp_coarse.py is the
// specification): which problems of an ICP stage first register a strided subsample, where the subsamples go in the source
// buffers, and which coarse result every problem of the fine stage starts from.  Plain inputs, plain outputs, no HIP runtime
// call and no context: icp_stage.hip feeds it from the context and issues the stream operations; icp_coarse_plan_check.cpp runs
// it on a CPU (tests/test_icp_coarse_cpu.py).  The hand-over predicate is here as well, for host and device: k_icp_coarse.hip
// applies it to the coarse state on the GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "common.hpp"

namespace cd {

constexpr int COARSE_STRIDE_MIN = 2, COARSE_STRIDE_MAX = 64;
constexpr int COARSE_REGION_ALIGN = 16;   // points: the coarse region starts on a 256-byte boundary of the source buffers

// cd_set_icp_coarse's argument rule: stride 0 (off; min_points is not looked at) or 2..64 with min_points >= 3 * stride, so that a
// coarse set never has fewer than three points
inline bool coarse_setting_ok(int stride, int min_points) {
    if (stride == 0) return true;
    return stride >= COARSE_STRIDE_MIN && stride <= COARSE_STRIDE_MAX && min_points >= 3 * stride;
}
inline bool coarse_eligible(int n, int stride, int min_points) { return stride >= COARSE_STRIDE_MIN && n >= min_points; }
inline int coarse_count(int n, int stride) { return (n + stride - 1) / stride; }

// cd_icp_coarse_subsample: the indices j * stride of an eligible set's coarse set; 0 when not eligible, the count otherwise
// (more than `capacity`: nothing was written)
inline int coarse_subsample(int n, int stride, int min_points, int32_t* out, int capacity) {
    if (n < 0 || !coarse_setting_ok(stride, min_points) || !coarse_eligible(n, stride, min_points)) return 0;
    const int nc = coarse_count(n, stride);
    if (out && nc <= capacity)
        for (int j = 0; j < nc; ++j) out[j] = j * stride;
    return nc;
}

// The points the source buffers must hold for the mode to fit any stage of a context of `fn` points: a coarse set has at most
// n / s + 1 <= n / s + n / (3 s) = 4 n / (3 s) <= 2 n / 3 points (n >= 3 s, s >= 2), and a stage's problems hold fn points at the most.
inline size_t coarse_source_capacity(size_t fn) { return fn + COARSE_REGION_ALIGN + (2 * fn + 2) / 3; }

// What the mode reports per (cluster, template) pair (cd_icp_coarse_stats)
struct CoarseStats {
    int32_t n_coarse;            // points of the coarse set (0: the pair was not eligible)
    int32_t coarse_iterations, coarse_converged;
    int32_t coarse_status;       // CD_OK, or why the coarse ICP stopped
    double coarse_fitness;       // of the coarse set under T_c
    int32_t used;                // 0 not eligible, 1 the fine level started from T_c, 2 fell back to the call's own guess
    int32_t reserved;
};
constexpr int COARSE_NOT_ELIGIBLE = 0, COARSE_USED = 1, COARSE_FELL_BACK = 2;

// One record per problem of the FINE stage, read by k_icp_coarse_handover: its coarse problem (-1: none) and that set's size
struct CoarseHand { int32_t coarse, n_coarse; };
// One record per coarse problem, read by k_icp_coarse_gather: dst[dst_off + j] = src[src_off + j * stride], j < n_coarse
struct CoarseGather { int32_t src_off, dst_off, n_coarse, stride; };

// Rule C18 step 4, on the final state of a coarse ICP: a stop (a status of its own, or - fewer than three correspondences, a
// singular C17 solve - converged = 0) or a non-finite entry of T_c sends the fine level back to the call's own guess.
// Returns the status the stats record shows (CD_OK: none) and sets *fall_back.
__host__ __device__ inline int coarse_handover(int status, int converged, const float* T, int* fall_back) {
    const int stop = status != CD_OK ? status : (converged ? CD_OK : CD_ERR_FEW_CORRESPONDENCES);
    bool finite = true;
    for (int i = 0; i < 16; ++i) finite = finite && (T[i] - T[i] == 0.f);   // (NaN and +-inf both fail)
    *fall_back = (stop != CD_OK || !finite) ? 1 : 0;
    return stop;
}

struct CoarsePlan {
    int n_eligible = 0;
    int max_n_coarse = 0;
    long long region_begin = 0, capacity_needed = 0;   // points: where the coarse region starts, and what the source buffers must hold
    std::vector<IcpCluster> coarse;                    // the coarse stage's problem list (src_off in the coarse region)
    std::vector<CoarseGather> gather;                  // one per coarse problem
    std::vector<CoarseHand> hand;                      // one per fine problem
};

// Problems cl[0..ncl) of a stage -> the coarse stage.  A problem is eligible when its set is (coarse_eligible) and it has a template
// to be matched against (the others are finished before they start: plan_icp marks them).  The coarse problems keep the order of
// their fine problems - so runs that share a template stay runs - and lie packed, one after the other, behind the last point any
// problem of the stage uses.  Returns CD_OK, or CD_ERR_CAPACITY when the region ends past `capacity` points (or past what an
// IcpCluster's offset can say); the plan then holds what was needed.
inline int plan_coarse(const IcpCluster* cl, int ncl, int stride, int min_points, long long capacity, CoarsePlan* pl) {
    *pl = CoarsePlan();
    pl->hand.assign((size_t)std::max(ncl, 0), CoarseHand{-1, 0});
    long long end = 0;
    for (int k = 0; k < ncl; ++k) end = std::max(end, (long long)cl[k].src_off + std::max(cl[k].n, 0));
    pl->region_begin = (end + COARSE_REGION_ALIGN - 1) / COARSE_REGION_ALIGN * COARSE_REGION_ALIGN;
    long long at = pl->region_begin;
    for (int k = 0; k < ncl; ++k) {
        if (!coarse_eligible(cl[k].n, stride, min_points) || cl[k].tpl_m <= 0) continue;
        const int nc = coarse_count(cl[k].n, stride);
        pl->hand[(size_t)k] = CoarseHand{pl->n_eligible, nc};
        pl->n_eligible += 1;
        pl->max_n_coarse = std::max(pl->max_n_coarse, nc);
        if (at + nc <= std::numeric_limits<int32_t>::max()) {
            IcpCluster cc = cl[k];
            cc.src_off = (int32_t)at;
            cc.n = nc;
            cc.tile0 = 0;
            pl->coarse.push_back(cc);
            pl->gather.push_back(CoarseGather{cl[k].src_off, (int32_t)at, nc, stride});
        }
        at += nc;
    }
    pl->capacity_needed = pl->n_eligible > 0 ? at : end;
    if (pl->n_eligible > 0 && (at > capacity || at > std::numeric_limits<int32_t>::max())) return CD_ERR_CAPACITY;
    return CD_OK;
}

}  // namespace cd
