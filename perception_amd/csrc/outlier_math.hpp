// outlier_math.hpp - the arithmetic of canonical rule C16 (perception_amd/outlier_filter.py is the specification):
// statistical outlier removal.  Steps 3 to 6 written once for host and device: the squared distance and its order-preserving
// key, the ascending double sum that gives a point's mean neighbour distance, the sequential sums and the statistics of a
// cloud, the decision.  k_outlier.hip runs it on the GPU, outlier_math_check.cpp on the CPU.  One correctly rounded IEEE
// operation per operator (the library's flags: no contraction, correctly rounded division and square root), so the result does
// not depend on who computes it.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace cd {

constexpr int OUTLIER_MAX_K = CD_OUTLIER_MAX_MEAN_K;   // mean_k + 1 best values of a query: one per lane of a wave
constexpr uint32_t OUTLIER_NO_KEY = 0xffffffffu;       // the key of "no candidate": above every squared distance, +inf included

// What the filter did to one cloud (a frame of a fused call, or the cloud of cd_outlier_filter)
struct OutlierRecord {
    int32_t n_before;      // points of the cloud
    int32_t n_finite;      // m
    int32_t n_kept;
    int32_t computed;      // 0: m <= mean_k, every finite point kept and the statistics 0
    double mean, stddev, threshold;
};

// step 1 (written so that a NaN fails)
__host__ __device__ inline bool outlier_finite(float x, float y, float z) {
    return (fabsf(x) <= 3.402823466e38f) && (fabsf(y) <= 3.402823466e38f) && (fabsf(z) <= 3.402823466e38f);
}

// step 3: (dx*dx + dy*dy) + dz*dz with d = candidate - query, as its bit pattern: non-negative floats order as their bits
__host__ __device__ inline uint32_t outlier_d2_key(float qx, float qy, float qz, float cx, float cy, float cz) {
    const float d2 = dist2(cx, cy, cz, qx, qy, qz);
    uint32_t k;
    __builtin_memcpy(&k, &d2, 4);
    return k;
}

// step 4: root_at(i), i = 1 .. mean_k, are the float32 square roots of the query's mean_k + 1 smallest squared distances in
// ascending order, the smallest (i = 0, the point itself) left out.  Root and sum are apart so that a wave takes the roots of
// all its lanes' keys at once and only the additions run in sequence.
__host__ __device__ inline float outlier_root(uint32_t key) {
    float d2;
    __builtin_memcpy(&d2, &key, 4);
    return rn_fsqrt(d2);
}
template <class RootAt>
__host__ __device__ inline float outlier_mean_dist(RootAt root_at, int mean_k) {
    double sum = 0.0;
    for (int i = 1; i <= mean_k; ++i) sum = rn_dadd(sum, (double)root_at(i));
    return (float)rn_ddiv(sum, (double)mean_k);
}

// step 5: the two sequential sums (a dropped point's dist is 0 and changes neither), then the statistics of m > mean_k points
struct OutlierSums { double sum, sq; };
__host__ __device__ inline void outlier_accumulate(OutlierSums& s, float dist) {
    const double d = (double)dist;
    s.sum = rn_dadd(s.sum, d);
    s.sq = rn_dadd(s.sq, rn_dmul(d, d));
}
__host__ __device__ inline void outlier_statistics(const OutlierSums& s, int m, double std_mul, OutlierRecord* r) {
    const double dm = (double)m;
    r->mean = rn_ddiv(s.sum, dm);
    const double var = rn_ddiv(rn_dsub(s.sq, rn_ddiv(rn_dmul(s.sum, s.sum), dm)), (double)(m - 1));
    r->stddev = rn_dsqrt(var);
    r->threshold = rn_dadd(r->mean, rn_dmul(std_mul, r->stddev));
}

// step 6, for a finite point of a cloud whose statistics were computed
__host__ __device__ inline bool outlier_keep(float dist, double threshold, int negative) {
    const bool inlier = (double)dist <= threshold;
    return negative ? !inlier : inlier;
}

}  // namespace cd
