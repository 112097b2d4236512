// overlay_math.hpp - steps 1, 3 and 4 of canonical rule C11, shared by the host entry cd_overlay_project and the
// projection kernel of k_overlay.hip so that both run the same sequence of correctly rounded operations.  On the device every
// operation is an explicit round-to-nearest intrinsic (no contraction can enter whatever the compile flags); the host build
// has -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "rn_ops.hpp"

namespace cd {

constexpr int OVERLAY_COORD_MAX = 8192;   // |pixel coordinate| of a drawn box, and the largest image side
constexpr int OVERLAY_MAX_THICKNESS = 64;

// step 1: corner k (order of icp.cpp:99-106) of cd_bbox_corners(pose, l, w, h), float32
__host__ __device__ inline void overlay_corner(const double* pose, const double* dims, int k, float c[3]) {
    const double sx = (k & 4) ? 1.0 : -1.0, sy = (k & 2) ? 1.0 : -1.0, sz = (k & 1) ? 1.0 : -1.0;
    const float x = (float)(rn_dmul(sx, dims[0]) / 2), y = (float)(rn_dmul(sy, dims[1]) / 2), z = (float)(rn_dmul(sz, dims[2]) / 2);
    for (int r = 0; r < 3; ++r) {
        const float h0 = (float)pose[4 * r], h1 = (float)pose[4 * r + 1], h2 = (float)pose[4 * r + 2], h3 = (float)pose[4 * r + 3];
        c[r] = rn_fadd(rn_fadd(rn_fadd(rn_fmul(h0, x), rn_fmul(h1, y)), rn_fmul(h2, z)), h3);
    }
}

// steps 3 and 4 for one corner: false when the corner makes its box a skipped one
__host__ __device__ inline bool overlay_pixel(const double* M, const float c[3], int32_t* u, int32_t* v) {
    const double x = (double)c[0], y = (double)c[1], z = (double)c[2];
    double h[3];
    for (int r = 0; r < 3; ++r)
        h[r] = rn_dadd(rn_dadd(rn_dadd(rn_dmul(M[4 * r], x), rn_dmul(M[4 * r + 1], y)), rn_dmul(M[4 * r + 2], z)), M[4 * r + 3]);
    const double fu = rn_ddiv(h[0], h[2]), fv = rn_ddiv(h[1], h[2]);
    const double lim = (double)(OVERLAY_COORD_MAX + 1);   // |trunc(a)| <= 8192  <=>  |a| < 8193
    // (written so that a NaN fails every comparison)
    if (!(h[2] > 0.0) || !(fu > -lim && fu < lim) || !(fv > -lim && fv < lim)) return false;
    *u = (int32_t)fu;   // truncation toward zero
    *v = (int32_t)fv;
    return true;
}

}  // namespace cd
