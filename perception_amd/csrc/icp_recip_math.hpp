// icp_recip_math.hpp - the arithmetic of canonical rule C22 (perception_amd/icp_reciprocal.py is the specification):
// reciprocal correspondences.  The reverse distance, the two running minima a query keeps over the source points before and from
// its own index, and the keep predicate, written once for host and device.  k_icp_recip.hip runs it on the GPU - the targets as
// LDS broadcasts - cd_icp_reciprocal_mask and icp_recip_math_check.cpp on the CPU.  Minima of float32 values and integer
// compares only, so the result does not depend on who computes it or in which order the targets are met.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "common.hpp"

namespace cd {

// What the mode reports per (cluster, template) pair (cd_icp_recip_stats)
struct RecipStats {
    KeptStats kept;
    int32_t last_n0;        // |K0| of the last iteration that looked for correspondences
    int32_t reserved[3];
};
static_assert(offsetof(RecipStats, last_n0) == offsetof(cd_icp_recip_stats, last_n0) &&
              offsetof(KeptStats, stopped_few) == offsetof(cd_icp_recip_stats, stopped_few), "RecipStats mirrors cd_icp_recip_stats");

// (step 2, d2(q, x) of a template point q and a source position x, is dist2(q, x): rn_ops.hpp)
// the running minimum over a set of targets (+inf: the empty set; a NaN distance never enters)
__host__ __device__ inline float recip_min(float best, float d) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_fminf(best, d);   // (v_min_f32; best is never a NaN, so this is the line below)
#else
    return d < best ? d : best;
#endif
}
// step 3 for query i with own = d2(q, X_i): before = the minimum over the sources i' < i, from = the minimum over i' >= i
// (own among them).  No earlier source is as near, no source at all is nearer.
__host__ __device__ inline bool recip_keep(float before, float from, float own) { return !(before <= own) && !(from < own); }

// Rule C5 by brute force on the host: nearest template point of (x, y, z), ties to the lowest index; m >= 1
inline int recip_forward_host(const float* tpl, size_t tpl_stride_f, int m, float x, float y, float z, float* d2_out) {
    int bj = 0;
    float best = std::numeric_limits<float>::infinity();
    for (int j = 0; j < m; ++j) {
        const float* t = tpl + (size_t)j * tpl_stride_f;
        const float d = dist2(x, y, z, t[0], t[1], t[2]);
        if (d < best || j == 0) { best = d; bj = j; }
    }
    *d2_out = best;
    return bj;
}

// Steps 1 - 3 on the host: keep[i] for the n source positions src (stride in floats) with rule C5's nn / d2 over the template.
// Returns |K0|; with fewer than three nothing is tested and keep is K0 itself.
inline int recip_mask_host(const float* src, size_t src_stride_f, int n, const float* tpl, size_t tpl_stride_f, float d2_max, const int32_t* nn,
                           const float* d2, uint8_t* keep) {
    int n0 = 0;
    for (int i = 0; i < n; ++i) { keep[i] = icp_in_k0(d2[i], d2_max) ? 1 : 0; n0 += keep[i]; }
    if (n0 < ICP_MIN_CORR) return n0;
    const float inf = std::numeric_limits<float>::infinity();
    for (int i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        const float* q = tpl + (size_t)nn[i] * tpl_stride_f;
        const float* xi = src + (size_t)i * src_stride_f;
        const float own = dist2(q[0], q[1], q[2], xi[0], xi[1], xi[2]);
        float before = inf, from = inf;
        for (int e = 0; e < n; ++e) {
            const float* x = src + (size_t)e * src_stride_f;
            const float d = dist2(q[0], q[1], q[2], x[0], x[1], x[2]);
            if (e < i) before = recip_min(before, d);
            else from = recip_min(from, d);
        }
        keep[i] = recip_keep(before, from, own) ? 1 : 0;
    }
    return n0;
}

}  // namespace cd
