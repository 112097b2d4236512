// label_math.hpp - the arithmetic of canonical rule C15 for one input point: rule C7's deprojection, the S0
// predicate, the point's voxel key in the two forms the voxel stage leaves its sorted keys in, the search for that key among a
// frame's voxel keys, the label of a voxel class, and the tint of one colour channel.  Host and device: k_labels.hip and
// k_depth.hip run it on the GPU, label_math_check.cpp against a plain double loop on the CPU.  One IEEE float32 operation per
// operator (the library's flags: no contraction, correctly rounded division).
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace cd {

constexpr int LABEL_INVALID = CD_LABEL_INVALID, LABEL_CROPPED = CD_LABEL_CROPPED, LABEL_PLANE = CD_LABEL_PLANE, LABEL_OBJECT = CD_LABEL_OBJECT,
              LABEL_GATED = CD_LABEL_GATED, LABEL_CLUSTER0 = CD_LABEL_CLUSTER0;
constexpr int LABEL_MAX_RANKS = 256 - LABEL_CLUSTER0;   // cluster ranks that have a label of their own: 0 .. 247

__host__ __device__ inline float label_qnan() {
    const uint32_t q = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &q, 4);
    return f;
}

// Rule C7: pixel (u, v) with depth value d -> x y z (quiet NaN for d == 0)
__host__ __device__ inline void deproject_c7(uint32_t u, uint32_t v, uint32_t d, float fx, float fy, float cx, float cy, float depth_scale,
                                             float* x, float* y, float* z) {
    if (d == 0u) {
        *x = *y = *z = label_qnan();
    } else {
        const float zz = (float)d * depth_scale;
        *x = (((float)u - cx) / fx) * zz;
        *y = (((float)v - cy) / fy) * zz;
        *z = zz;
    }
}

__host__ __device__ inline bool label_finite(float x, float y, float z) {
    return (fabsf(x) <= 3.402823466e38f) && (fabsf(y) <= 3.402823466e38f) && (fabsf(z) <= 3.402823466e38f);
}
// the S0 predicate of a finite point (k_voxel.hip crop_keep): the z limits, then the x limits, both inclusive
__host__ __device__ inline bool label_kept(float x, float z, const CropLimits& L) { return z >= L.zlo && z <= L.zhi && x >= L.xlo && x <= L.xhi; }

// floor(v * inv_leaf) as an int, when it is one below 2^31 in magnitude (a finite v can still overflow the product)
__host__ __device__ inline bool label_cell(float v, float inv, float* fl, int* cell) {
    *fl = floorf(v * inv);
    if (!(fabsf(*fl) < 2.0e9f)) return false;
    *cell = (int)*fl;
    return true;
}

// The point's key as k_crop_runs packs it (packed_cell_key, k_voxel.hip): x | y << bi | z << (bi + bj), every field the cell
// coordinate less the field's low end.  false: a coordinate does not fit its field - no voxel of the call can have that key.
__host__ __device__ inline bool label_key_packed(float x, float y, float z, float inv, const KeyPack& kp, uint32_t* key) {
    float f;
    int ci, cj, ck;
    if (!label_cell(x, inv, &f, &ci) || !label_cell(y, inv, &f, &cj) || !label_cell(z, inv, &f, &ck)) return false;
    const int bk = 32 - kp.bi - kp.bj;
    const long long ui = (long long)ci - kp.ilo, uj = (long long)cj - kp.jlo, uk = (long long)ck - kp.klo;
    if (ui < 0 || ui >= (1ll << kp.bi) || uj < 0 || uj >= (1ll << kp.bj) || uk < 0 || uk >= (1ll << bk)) return false;
    *key = (uint32_t)ui | ((uint32_t)uj << kp.bi) | ((uint32_t)uk << (kp.bi + kp.bj));
    return true;
}

// The point's key as PCL's VoxelGrid numbers the cell: ijk = (int)(floor(p * inv_leaf) - min_b) in float32, idx = i + j dx +
// k dx dy.  false: the cell lies outside the frame's grid (the index is never formed, let alone used).
struct LabelGrid { int32_t min_b[3], div_b[3]; };
__host__ __device__ inline bool label_key_idx(float x, float y, float z, float inv, const LabelGrid& g, uint32_t* key) {
    const float p[3] = {x, y, z};
    int ijk[3];
    for (int a = 0; a < 3; ++a) {
        const float d = floorf(p[a] * inv) - (float)g.min_b[a];
        if (!(d >= 0.f && d < 2.0e9f)) return false;
        ijk[a] = (int)d;
        if (ijk[a] >= g.div_b[a]) return false;
    }
    // (inside the grid: idx < dx dy dz <= 2^31 - 1, which k_voxel_setup checked)
    *key = (uint32_t)(ijk[0] + ijk[1] * g.div_b[0] + ijk[2] * (g.div_b[0] * g.div_b[1]));
    return true;
}

// First position of keys[0, n) (ascending, distinct) whose key is not below `key`; at most 32 probes, none outside [0, n)
__host__ __device__ inline int label_lower_bound(const uint32_t* keys, int n, uint32_t key) {
    int lo = 0, hi = n > 0 ? n : 0;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The same for K keys at once, each in a table of its own, the K searches in step: every round issues the K probes together
// (independent loads in flight at once instead of K chains of dependent ones).  keys[k] must point to at least one readable
// word even when n[k] <= 0 (a search that is over probes word 0 and ignores it); at[k] as label_lower_bound returns it.
template <int K>
__host__ __device__ inline void label_lower_bound_n(const uint32_t* const (&keys)[K], const int (&n)[K], const uint32_t (&key)[K], int (&at)[K]) {
    int lo[K], len[K], live = 0;
    for (int k = 0; k < K; ++k) { lo[k] = 0; len[k] = n[k] > 0 ? n[k] : 0; live |= len[k]; }
    for (int it = 0; it < 32 && live; ++it) {
        uint32_t v[K];
        int mid[K];
        for (int k = 0; k < K; ++k) {
            mid[k] = lo[k] + (len[k] >> 1);          // (inside [lo, lo + len) while len > 0)
            v[k] = keys[k][len[k] > 0 ? mid[k] : 0];
        }
        live = 0;
        for (int k = 0; k < K; ++k) {
            if (len[k] > 0) {
                const int half = len[k] >> 1;
                if (v[k] < key[k]) { lo[k] = mid[k] + 1; len[k] -= half + 1; } else len[k] = half;
            }
            live |= len[k];
        }
    }
    for (int k = 0; k < K; ++k) at[k] = lo[k];
}

// class of an object voxel from its cluster label (d_label: -1 = in no cluster that was kept)
__host__ __device__ inline uint8_t label_of_rank(int rank) {
    return (uint8_t)((rank >= 0 && rank < LABEL_MAX_RANKS) ? LABEL_CLUSTER0 + rank : LABEL_OBJECT);
}

// one channel of cd_tint_labels_batch: (c (255 - a) + p a + 127) / 255 in integers
__host__ __device__ inline uint8_t label_tint(uint32_t c, uint32_t p, uint32_t a) { return (uint8_t)((c * (255u - a) + p * a + 127u) / 255u); }

}  // namespace cd
