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

#ifdef __HIP_DEVICE_COMPILE__
#define CD_OL_FSUB(a, b) __fsub_rn((a), (b))
#define CD_OL_FMUL(a, b) __fmul_rn((a), (b))
#define CD_OL_FADD(a, b) __fadd_rn((a), (b))
#define CD_OL_FSQRT(a) sqrtf((a))   // (IEEE under -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is the native approximation)
#define CD_OL_MUL(a, b) __dmul_rn((a), (b))
#define CD_OL_ADD(a, b) __dadd_rn((a), (b))
#define CD_OL_SUB(a, b) __dsub_rn((a), (b))
#define CD_OL_DIV(a, b) __ddiv_rn((a), (b))
#define CD_OL_SQRT(a) __dsqrt_rn((a))
#else
#define CD_OL_FSUB(a, b) ((a) - (b))
#define CD_OL_FMUL(a, b) ((a) * (b))
#define CD_OL_FADD(a, b) ((a) + (b))
#define CD_OL_FSQRT(a) std::sqrt((a))
#define CD_OL_MUL(a, b) ((a) * (b))
#define CD_OL_ADD(a, b) ((a) + (b))
#define CD_OL_SUB(a, b) ((a) - (b))
#define CD_OL_DIV(a, b) ((a) / (b))
#define CD_OL_SQRT(a) std::sqrt((a))
#endif

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
    const float dx = CD_OL_FSUB(cx, qx), dy = CD_OL_FSUB(cy, qy), dz = CD_OL_FSUB(cz, qz);
    const float d2 = CD_OL_FADD(CD_OL_FADD(CD_OL_FMUL(dx, dx), CD_OL_FMUL(dy, dy)), CD_OL_FMUL(dz, dz));
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
    return CD_OL_FSQRT(d2);
}
template <class RootAt>
__host__ __device__ inline float outlier_mean_dist(RootAt root_at, int mean_k) {
    double sum = 0.0;
    for (int i = 1; i <= mean_k; ++i) sum = CD_OL_ADD(sum, (double)root_at(i));
    return (float)CD_OL_DIV(sum, (double)mean_k);
}

// step 5: the two sequential sums (a dropped point's dist is 0 and changes neither), then the statistics of m > mean_k points
struct OutlierSums { double sum, sq; };
__host__ __device__ inline void outlier_accumulate(OutlierSums& s, float dist) {
    const double d = (double)dist;
    s.sum = CD_OL_ADD(s.sum, d);
    s.sq = CD_OL_ADD(s.sq, CD_OL_MUL(d, d));
}
__host__ __device__ inline void outlier_statistics(const OutlierSums& s, int m, double std_mul, OutlierRecord* r) {
    const double dm = (double)m;
    r->mean = CD_OL_DIV(s.sum, dm);
    const double var = CD_OL_DIV(CD_OL_SUB(s.sq, CD_OL_DIV(CD_OL_MUL(s.sum, s.sum), dm)), (double)(m - 1));
    r->stddev = CD_OL_SQRT(var);
    r->threshold = CD_OL_ADD(r->mean, CD_OL_MUL(std_mul, r->stddev));
}

// step 6, for a finite point of a cloud whose statistics were computed
__host__ __device__ inline bool outlier_keep(float dist, double threshold, int negative) {
    const bool inlier = (double)dist <= threshold;
    return negative ? !inlier : inlier;
}

}  // namespace cd
