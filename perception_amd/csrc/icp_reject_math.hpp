// icp_reject_math.hpp - the arithmetic of canonical rule C19 (perception_amd/icp_reject.py is the specification):
// median-distance correspondence rejection.  The exact rank selection on the bits of the float32 squared distances (non-negative
// floats order as their unsigned bits, +inf included; rule C5 never yields a NaN or a negative zero), the threshold and the keep
// predicate, written once for host and device.  k_icp_reject.hip runs it on the GPU - the histogram of a round in LDS, the prefix
// by one wave - cd_icp_median_threshold and icp_reject_math_check.cpp on the CPU.  The selection is integer work and the
// threshold ONE rounded double product, so the result does not depend on who computes it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace cd {

constexpr int REJECT_DIGIT_BITS = 8;                       // the key's 32 bits go in four rounds, most significant digit first
constexpr int REJECT_BINS = 1 << REJECT_DIGIT_BITS;
constexpr int REJECT_ROUNDS = 32 / REJECT_DIGIT_BITS;

// What the mode reports per (cluster, template) pair (cd_icp_reject_stats)
struct RejectStats {
    KeptStats kept;
    float last_median;      // m of the last iteration that selected one (0: none did)
    int32_t reserved[3];
};
static_assert(offsetof(RejectStats, last_median) == offsetof(cd_icp_reject_stats, last_median) &&
              offsetof(KeptStats, stopped_few) == offsetof(cd_icp_reject_stats, stopped_few), "RejectStats mirrors cd_icp_reject_stats");

__host__ __device__ inline uint32_t reject_key(float d2) {
    uint32_t k;
    __builtin_memcpy(&k, &d2, 4);
    return k;
}
__host__ __device__ inline float reject_value(uint32_t key) {
    float v;
    __builtin_memcpy(&v, &key, 4);
    return v;
}
// round r = 0 .. 3 looks at the keys whose r leading digits equal `prefix` (r = 0: all of them) and counts digit r
__host__ __device__ inline bool reject_in_round(uint32_t key, uint32_t prefix, int r) {
    return r == 0 || (key >> (32 - REJECT_DIGIT_BITS * r)) == prefix;
}
__host__ __device__ inline uint32_t reject_digit(uint32_t key, int r) {
    return (key >> (32 - REJECT_DIGIT_BITS * (r + 1))) & (uint32_t)(REJECT_BINS - 1);
}
// step 2's rank among n0 survivors of rule C8's bound: the upper median
__host__ __device__ inline uint32_t reject_rank(uint32_t n0) { return n0 / 2u; }
// step 3
__host__ __device__ inline double reject_threshold(float m, double factor) { return rn_dmul((double)m, factor); }
// step 4 (for a correspondence of K0)
__host__ __device__ inline bool reject_keep(float d2, double thr) { return (double)d2 <= thr; }

// The bin of a round's histogram that holds rank `rank` (0-based among the counted keys), and the rank inside that bin.
// Sequential form (host; the device's wave does the same prefix in parallel).  The counts sum to more than `rank`.
inline uint32_t reject_pick_bin(const uint32_t* hist, uint32_t rank, uint32_t* rank_in) {
    uint32_t below = 0;
    for (uint32_t b = 0; b < (uint32_t)REJECT_BINS; ++b) {
        if (rank < below + hist[b]) { *rank_in = rank - below; return b; }
        below += hist[b];
    }
    *rank_in = 0;
    return (uint32_t)REJECT_BINS - 1u;   // (not reached with counts that sum to more than rank)
}

// Steps 2 and 3 on the host over the n0 >= 1 values of K0, by the same four histogram rounds as the kernel.
inline void reject_median_host(const float* d2_k0, uint32_t n0, double factor, float* median, double* thr) {
    uint32_t prefix = 0, rank = reject_rank(n0);
    for (int r = 0; r < REJECT_ROUNDS; ++r) {
        uint32_t hist[REJECT_BINS] = {0};
        for (uint32_t i = 0; i < n0; ++i) {
            const uint32_t k = reject_key(d2_k0[i]);
            if (reject_in_round(k, prefix, r)) hist[reject_digit(k, r)] += 1u;
        }
        uint32_t in = 0;
        const uint32_t b = reject_pick_bin(hist, rank, &in);
        prefix = (prefix << REJECT_DIGIT_BITS) | b;
        rank = in;
    }
    *median = reject_value(prefix);
    *thr = reject_threshold(*median, factor);
}

}  // namespace cd
