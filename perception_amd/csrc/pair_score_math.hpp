// pair_score_math.hpp - the arithmetic of canonical rule C21 (perception_amd/pair_score.py is the specification): the
// two-way registration score of a (cluster, template) pair.  The single evaluation of T on a point, the squared distance, the
// clamped fixed-point term, the finiteness test and the record built from the integer sums, written once for host and device.
// k_pair_score.hip runs the all-pairs minima on the GPU, pair_score_host below on the CPU (cd_pair_score_host,
// pair_score_math_check.cpp); both hand the same six integers to pair_record.  Every float32 operation is one IEEE operation
// (rule C1); the minima, counts and sums are order-free, so the result does not depend on who computes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "common.hpp"

namespace cd {

constexpr float PAIR_TERM_MAX = 256.0f;   // step 5: a term of a sum is min(d2, 256): fixq(., 36) <= 2^44, 2^19 of them <= 2^63
constexpr int PAIR_MAX_POINTS = 1 << 19;  // rule C4's N
constexpr int PAIR_MIN_SOURCE = 3;

// the integers a pair's two passes leave (one row of the kernel's accumulator)
enum { PAIR_N_SRC_IN = 0, PAIR_N_TPL_IN = 1, PAIR_S_FWD_IN = 2, PAIR_S_REV_IN = 3, PAIR_S_REV_ALL = 4, PAIR_BAD = 5, PAIR_ACC_PITCH = 8 };

// (step 1, the single evaluation of T on a point, is xform_row and step 2 is dist2: rn_ops.hpp)
// step 5: rint(min(v, 256) 2^36), v >= 0 or +inf
__host__ __device__ inline unsigned long long pair_term(float v) {
    const float t = v < PAIR_TERM_MAX ? v : PAIR_TERM_MAX;
#ifdef __HIP_DEVICE_COMPILE__
    return (unsigned long long)__double2ll_rn(ldexp((double)t, FIX_SHIFT_D2));
#else
    return (unsigned long long)std::llrint(std::ldexp((double)t, FIX_SHIFT_D2));
#endif
}
__host__ __device__ inline bool pair_finite(float x, float y, float z) {
    uint32_t b[3];
    __builtin_memcpy(&b[0], &x, 4); __builtin_memcpy(&b[1], &y, 4); __builtin_memcpy(&b[2], &z, 4);
    return (b[0] & 0x7f800000u) != 0x7f800000u && (b[1] & 0x7f800000u) != 0x7f800000u && (b[2] & 0x7f800000u) != 0x7f800000u;
}

// rule C8's tau for pair_score_math_check.cpp, which links no library: cd_icp_correspondence_threshold's arithmetic (the library's
// own calls go through that function)
inline float pair_tau(double d) {
    const double dd = d * d;
    float f = (float)dd;
    if ((double)f > dd) f = std::nextafter(f, 0.f);
    return f;
}
inline bool pair_thresholds_ok(double d, double min_cov, double min_inl) {
    return std::isfinite(d) && d > 0.0 && min_cov >= 0.0 && min_cov <= 1.0 && min_inl >= 0.0 && min_inl <= 1.0;   // (a NaN fails)
}
// step 8 as far as it can be told without the points: CD_OK means "run the passes"
inline int pair_pre_status(int n, int m, const float* T) {
    if (m <= 0) return CD_ERR_NO_TEMPLATE;
    if (n < PAIR_MIN_SOURCE) return CD_ERR_FEW_CORRESPONDENCES;
    if (n > PAIR_MAX_POINTS || m > PAIR_MAX_POINTS) return CD_ERR_CAPACITY;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(T[i])) return CD_ERR_INVALID_ARG;
    return CD_OK;
}
// steps 5 - 8: the record from the pre-status and (pre-status CD_OK) the six integers of the passes
inline void pair_record(int n, int m, int pre_status, const unsigned long long* acc, int accepted, double min_cov, double min_inl, cd_pair_score* out) {
    std::memset(out, 0, sizeof(*out));
    out->n_source = n;
    out->n_template = std::max(m, 0);
    out->status = pre_status;
    if (pre_status != CD_OK) return;
    if (acc[PAIR_BAD] != 0ull) { out->status = CD_ERR_INVALID_ARG; return; }
    const double q = std::ldexp(1.0, -FIX_SHIFT_D2);
    out->n_source_in = (int32_t)acc[PAIR_N_SRC_IN];
    out->n_template_in = (int32_t)acc[PAIR_N_TPL_IN];
    out->forward_fitness_in = out->n_source_in > 0 ? ((double)acc[PAIR_S_FWD_IN] * q) / (double)out->n_source_in : 0.0;
    out->reverse_fitness_in = out->n_template_in > 0 ? ((double)acc[PAIR_S_REV_IN] * q) / (double)out->n_template_in : 0.0;
    out->reverse_fitness = ((double)acc[PAIR_S_REV_ALL] * q) / (double)m;
    out->coverage = (double)out->n_template_in / (double)m;
    out->inlier_fraction = (double)out->n_source_in / (double)n;
    out->valid = (accepted && out->coverage >= min_cov && out->inlier_fraction >= min_inl) ? 1 : 0;
}

// The passes on the host: tpl and src are m and n tightly packed xyz triples, pre_status has been CD_OK.  acc: PAIR_ACC_PITCH words.
inline void pair_passes_host(const float* tpl, int m, const float* src, int n, const float* T, float tau, unsigned long long* acc) {
    for (int i = 0; i < PAIR_ACC_PITCH; ++i) acc[i] = 0ull;
    float* A = new float[(size_t)n * 3];
    for (int i = 0; i < n; ++i) {
        for (int r = 0; r < 3; ++r) A[3 * (size_t)i + r] = xform_row(T, r, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
        if (!pair_finite(A[3 * (size_t)i], A[3 * (size_t)i + 1], A[3 * (size_t)i + 2])) acc[PAIR_BAD] += 1ull;
    }
    for (int j = 0; j < m; ++j)
        if (!pair_finite(tpl[3 * (size_t)j], tpl[3 * (size_t)j + 1], tpl[3 * (size_t)j + 2])) acc[PAIR_BAD] += 1ull;
    if (acc[PAIR_BAD] == 0ull) {
        const float inf = INFINITY;
        for (int i = 0; i < n; ++i) {
            float best = inf;
            for (int j = 0; j < m; ++j) {
                const float v = dist2(A[3 * (size_t)i], A[3 * (size_t)i + 1], A[3 * (size_t)i + 2], tpl[3 * (size_t)j], tpl[3 * (size_t)j + 1], tpl[3 * (size_t)j + 2]);
                best = v < best ? v : best;
            }
            if (best <= tau) { acc[PAIR_N_SRC_IN] += 1ull; acc[PAIR_S_FWD_IN] += pair_term(best); }
        }
        for (int j = 0; j < m; ++j) {
            float best = inf;
            for (int i = 0; i < n; ++i) {
                const float v = dist2(tpl[3 * (size_t)j], tpl[3 * (size_t)j + 1], tpl[3 * (size_t)j + 2], A[3 * (size_t)i], A[3 * (size_t)i + 1], A[3 * (size_t)i + 2]);
                best = v < best ? v : best;
            }
            if (best <= tau) { acc[PAIR_N_TPL_IN] += 1ull; acc[PAIR_S_REV_IN] += pair_term(best); }
            acc[PAIR_S_REV_ALL] += pair_term(best);
        }
    }
    delete[] A;
}

}  // namespace cd
