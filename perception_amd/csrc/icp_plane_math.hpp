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
constexpr int PLANE_MIN_CORR = 3;            // (ICP_MIN_CORR: fewer kept correspondences stop the ICP before the update)
constexpr double PLANE_SINGULAR_EPS = 9.094947017729282379150390625e-13;   // 2^-40

#ifdef __HIP_DEVICE_COMPILE__
#define CD_PL_FSUB(a, b) __fsub_rn((a), (b))
#define CD_PL_FMUL(a, b) __fmul_rn((a), (b))
#define CD_PL_MUL(a, b) __dmul_rn((a), (b))
#define CD_PL_ADD(a, b) __dadd_rn((a), (b))
#define CD_PL_SUB(a, b) __dsub_rn((a), (b))
#define CD_PL_DIV(a, b) __ddiv_rn((a), (b))
#else
#define CD_PL_FSUB(a, b) ((a) - (b))
#define CD_PL_FMUL(a, b) ((a) * (b))
#define CD_PL_MUL(a, b) ((a) * (b))
#define CD_PL_ADD(a, b) ((a) + (b))
#define CD_PL_SUB(a, b) ((a) - (b))
#define CD_PL_DIV(a, b) ((a) / (b))
#endif

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
        const float r = CD_PL_FSUB(q[a], s[a]);
        const float g = a == w ? 1.0f : lam_it;
        const float u = CD_PL_FMUL(g, s[c]), v = CD_PL_FMUL(g, s[b]), h = CD_PL_FMUL(g, r);
        out[9 * a + 0] = g;
        out[9 * a + 1] = u;
        out[9 * a + 2] = v;
        out[9 * a + 3] = CD_PL_FMUL(u, s[c]);
        out[9 * a + 4] = CD_PL_FMUL(v, s[b]);
        out[9 * a + 5] = CD_PL_FMUL(u, s[b]);
        out[9 * a + 6] = h;
        out[9 * a + 7] = CD_PL_FMUL(h, s[c]);
        out[9 * a + 8] = CD_PL_FMUL(h, s[b]);
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
        M[b][b] = CD_PL_ADD(M[b][b], S[3]);
        M[c][c] = CD_PL_ADD(M[c][c], S[4]);
        M[hi][lo] = CD_PL_ADD(M[hi][lo], -S[5]);
        M[3 + a][b] = CD_PL_ADD(M[3 + a][b], S[1]);
        M[3 + a][c] = CD_PL_ADD(M[3 + a][c], -S[2]);
        M[3 + a][3 + a] = CD_PL_ADD(M[3 + a][3 + a], S[0]);
        rhs[b] = CD_PL_ADD(rhs[b], S[7]);
        rhs[c] = CD_PL_ADD(rhs[c], -S[8]);
        rhs[3 + a] = CD_PL_ADD(rhs[3 + a], S[6]);
    }
    double L[6][6], W[6][6], d[6];
    int singular = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double acc = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) acc = CD_PL_SUB(acc, CD_PL_MUL(W[j][k], L[j][k]));
        d[j] = acc;
        if (!(acc > CD_PL_MUL(M[j][j], PLANE_SINGULAR_EPS))) singular = 1;
        // (a singular column's quotients are never used: the result is the identity.  They are still computed - the loops
        // have no early exit, so that they unroll - and may be infinite or NaN.)
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) w = CD_PL_SUB(w, CD_PL_MUL(W[i][k], L[j][k]));
            W[i][j] = w;
            L[i][j] = CD_PL_DIV(w, acc);
        }
    }
    if (singular) return 1;
    double y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double acc = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) acc = CD_PL_SUB(acc, CD_PL_MUL(L[i][k], y[k]));
        y[i] = acc;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double acc = CD_PL_DIV(y[i], d[i]);
#pragma unroll
        for (int k = 5; k > i; --k) acc = CD_PL_SUB(acc, CD_PL_MUL(L[k][i], x[k]));
        x[i] = acc;
    }
    const double kx = CD_PL_MUL(x[0], 0.5), ky = CD_PL_MUL(x[1], 0.5), kz = CD_PL_MUL(x[2], 0.5);
    const double xx = CD_PL_MUL(kx, kx), yy = CD_PL_MUL(ky, ky), zz = CD_PL_MUL(kz, kz);
    const double m = CD_PL_ADD(CD_PL_ADD(CD_PL_ADD(1.0, xx), yy), zz);
    const double xy = CD_PL_MUL(kx, ky), xz = CD_PL_MUL(kx, kz), yz = CD_PL_MUL(ky, kz);
    T[0] = (float)CD_PL_DIV(CD_PL_SUB(CD_PL_SUB(CD_PL_ADD(1.0, xx), yy), zz), m);
    T[1] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_SUB(xy, kz)), m);
    T[2] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_ADD(xz, ky)), m);
    T[4] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_ADD(xy, kz)), m);
    T[5] = (float)CD_PL_DIV(CD_PL_SUB(CD_PL_ADD(CD_PL_SUB(1.0, xx), yy), zz), m);
    T[6] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_SUB(yz, kx)), m);
    T[8] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_SUB(xz, ky)), m);
    T[9] = (float)CD_PL_DIV(CD_PL_MUL(2.0, CD_PL_ADD(yz, kx)), m);
    T[10] = (float)CD_PL_DIV(CD_PL_ADD(CD_PL_SUB(CD_PL_SUB(1.0, xx), yy), zz), m);
    T[3] = (float)x[3]; T[7] = (float)x[4]; T[11] = (float)x[5];
    return 0;
}

}  // namespace cd
