// icp_plane_math.hpp - the arithmetic of canonical rule C17 (perception_amd/icp_plane.py is the specification):
// the plane-weighted ICP step for lattice templates.  Written once for host and device: the 27 float32 terms of one
// correspondence (plus d2), rule C4's conversion, and the solve - assembly of the 6 x 6 normal equations from the 28 integer
// sums, the square-root-free Cholesky factorisation (L D L^T) with its singularity test, the two substitutions and the rotation
// of the quaternion (1, omega / 2) as polynomials divided by its squared norm.  k_icp_plane.hip runs it on the GPU,
// cd_icp_plane_solve_host and icp_plane_math_check.cpp on the CPU.  One correctly rounded IEEE operation per operator (the
// library's flags: no contraction), no square root and no library function, so the result does not depend on who computes it.
// This is NOT pcl::registration::TransformationEstimationPointToPlaneLLS: that estimator is the case lambda = 0, which is
// singular whenever the correspondences touch two faces only.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace cd {

constexpr int PLANE_NSUMS = 28;              // 9 per axis, then d2
constexpr double PLANE_SINGULAR_EPS = 9.094947017729282379150390625e-13;   // 2^-40

// What the mode reports per (cluster, template) pair (cd_icp_plane_stats)
struct PlaneStats {
    int32_t plane_iterations;        // iterations run with the latch closed (tangential weight = tangent_weight)
    int32_t first_plane_iteration;   // the first of them, 1-based; 0: never latched
    int32_t stopped_singular;        // the ICP stopped before an update because the step's system was singular
    int32_t reserved;
};

// The setting as the kernel takes it
struct PlaneParams {
    float lambda;        // (float)tangent_weight
    int32_t latched0;    // switch_distance == +inf: plane weights from the first iteration
    double switch2;      // switch_distance * switch_distance (one double multiply)
};

// rule C17 step 2: the 27 terms of a correspondence - s the moved source point, q its template point, w the constant axis of
// q's face, lam_it this iteration's tangential weight - and d2 in out[27].  out[9 a + j]: term j of axis a.
__host__ __device__ inline void plane_terms(const float (&s)[3], const float (&q)[3], int w, float lam_it, float d2, float (&out)[PLANE_NSUMS]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const float r = rn_fsub(q[a], s[a]);
        const float g = a == w ? 1.0f : lam_it;
        const float u = rn_fmul(g, s[c]), v = rn_fmul(g, s[b]), h = rn_fmul(g, r);
        out[9 * a + 0] = g;
        out[9 * a + 1] = u;
        out[9 * a + 2] = v;
        out[9 * a + 3] = rn_fmul(u, s[c]);
        out[9 * a + 4] = rn_fmul(v, s[b]);
        out[9 * a + 5] = rn_fmul(u, s[b]);
        out[9 * a + 6] = h;
        out[9 * a + 7] = rn_fmul(h, s[c]);
        out[9 * a + 8] = rn_fmul(h, s[b]);
    }
    out[27] = d2;
}

// rule C4's conversion rint(v * 2^shift), ties to even (the device's fixq; the host rounds in the default rounding mode)
__host__ __device__ inline long long plane_fix(float v, int shift) {
#ifdef __HIP_DEVICE_COMPILE__
    return __double2ll_rn(ldexp((double)v, shift));
#else
    return std::llrint(std::ldexp((double)v, shift));
#endif
}
__host__ __device__ inline int plane_shift(int i) { return i == 27 ? FIX_SHIFT_D2 : FIX_SHIFT; }

__host__ __device__ inline double plane_unfix(long long s, int shift) { return ldexp((double)s, -shift); }

// rule C17 steps 3 and 4: T (row-major 4 x 4, float32) from the 28 sums; returns 1 and the identity when the system is
// singular (or n < 1).  Every loop has constant bounds and is unrolled: the matrices live in registers on the device.
__host__ __device__ inline int plane_solve(const long long* A, int n, float* T) {
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f;
    if (n < 1) return 1;
    double M[6][6], rhs[6];   // lower triangle: M[i][j], i >= j
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        rhs[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) M[i][j] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const int hi = b > c ? b : c, lo = b > c ? c : b;
        double S[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) S[j] = plane_unfix(A[9 * a + j], FIX_SHIFT);
        M[b][b] = rn_dadd(M[b][b], S[3]);
        M[c][c] = rn_dadd(M[c][c], S[4]);
        M[hi][lo] = rn_dadd(M[hi][lo], -S[5]);
        M[3 + a][b] = rn_dadd(M[3 + a][b], S[1]);
        M[3 + a][c] = rn_dadd(M[3 + a][c], -S[2]);
        M[3 + a][3 + a] = rn_dadd(M[3 + a][3 + a], S[0]);
        rhs[b] = rn_dadd(rhs[b], S[7]);
        rhs[c] = rn_dadd(rhs[c], -S[8]);
        rhs[3 + a] = rn_dadd(rhs[3 + a], S[6]);
    }
    double L[6][6], W[6][6], d[6];
    int singular = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double acc = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) acc = rn_dsub(acc, rn_dmul(W[j][k], L[j][k]));
        d[j] = acc;
        if (!(acc > rn_dmul(M[j][j], PLANE_SINGULAR_EPS))) singular = 1;
        // (a singular column's quotients are never used: the result is the identity.  They are still computed - the loops
        // have no early exit, so that they unroll - and may be infinite or NaN.)
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) w = rn_dsub(w, rn_dmul(W[i][k], L[j][k]));
            W[i][j] = w;
            L[i][j] = rn_ddiv(w, acc);
        }
    }
    if (singular) return 1;
    double y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double acc = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) acc = rn_dsub(acc, rn_dmul(L[i][k], y[k]));
        y[i] = acc;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double acc = rn_ddiv(y[i], d[i]);
#pragma unroll
        for (int k = 5; k > i; --k) acc = rn_dsub(acc, rn_dmul(L[k][i], x[k]));
        x[i] = acc;
    }
    const double kx = rn_dmul(x[0], 0.5), ky = rn_dmul(x[1], 0.5), kz = rn_dmul(x[2], 0.5);
    const double xx = rn_dmul(kx, kx), yy = rn_dmul(ky, ky), zz = rn_dmul(kz, kz);
    const double m = rn_dadd(rn_dadd(rn_dadd(1.0, xx), yy), zz);
    const double xy = rn_dmul(kx, ky), xz = rn_dmul(kx, kz), yz = rn_dmul(ky, kz);
    T[0] = (float)rn_ddiv(rn_dsub(rn_dsub(rn_dadd(1.0, xx), yy), zz), m);
    T[1] = (float)rn_ddiv(rn_dmul(2.0, rn_dsub(xy, kz)), m);
    T[2] = (float)rn_ddiv(rn_dmul(2.0, rn_dadd(xz, ky)), m);
    T[4] = (float)rn_ddiv(rn_dmul(2.0, rn_dadd(xy, kz)), m);
    T[5] = (float)rn_ddiv(rn_dsub(rn_dadd(rn_dsub(1.0, xx), yy), zz), m);
    T[6] = (float)rn_ddiv(rn_dmul(2.0, rn_dsub(yz, kx)), m);
    T[8] = (float)rn_ddiv(rn_dmul(2.0, rn_dsub(xz, ky)), m);
    T[9] = (float)rn_ddiv(rn_dmul(2.0, rn_dadd(yz, kx)), m);
    T[10] = (float)rn_ddiv(rn_dadd(rn_dsub(rn_dsub(1.0, xx), yy), zz), m);
    T[3] = (float)x[3]; T[7] = (float)x[4]; T[11] = (float)x[5];
    return 0;
}

}  // namespace cd
