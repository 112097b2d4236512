// shape_frame_math.hpp - steps 1b to 5 of canonical rule C13: from the nine fixed-point moment sums of a point
// set to its principal frame, the projection of a point on that frame, and the rigid guess that carries a cluster's frame onto
// a template's.  Shared by the host entries (cd_shape_frame_host, cd_shape_guess, cd_set_template's slot record) and by
// k_shape.hip so that both run the same sequence of correctly rounded double operations.  On the device every operation is an
// explicit round-to-nearest intrinsic (no contraction can enter whatever the compile flags); the host build has
// -ffp-contract=off.  Only + - x / sqrt and comparisons: perception_amd/cluster_frame.py reproduces every bit with Python floats.
#pragma once
#include <cmath>
#include <cstdint>

#include "rn_ops.hpp"

namespace cd {

constexpr int SHAPE_SWEEPS = 8;            // cyclic Jacobi sweeps, fixed
constexpr int SHAPE_N_MAX = 1 << 19;       // rule C4's count
constexpr float SHAPE_COORD_MAX = 64.f;    // rule C4's range
constexpr int SHAPE_OK = 0, SHAPE_ERR_INVALID = -1, SHAPE_ERR_CAPACITY = -2, SHAPE_ERR_FEW = -5;   // = CD_OK, CD_ERR_INVALID_ARG, CD_ERR_CAPACITY, CD_ERR_FEW_CORRESPONDENCES

struct ShapeFrame {          // = cd_shape_frame
    int32_t n, status;
    double mean[3];
    double axes[9];          // row-major, columns = axes
    double var[3];
    double lo[3], hi[3];
};

// the point may enter a set: finite and inside rule C4's range
__host__ __device__ inline bool shape_coord_ok(float x, float y, float z) {
    // (written so that a NaN fails)
    return fabsf(x) <= SHAPE_COORD_MAX && fabsf(y) <= SHAPE_COORD_MAX && fabsf(z) <= SHAPE_COORD_MAX;
}

// one Jacobi rotation of the pair (P, Q); R is the third index.  a: symmetric 3x3 (all nine entries kept), v: the rotations so far
template <int P, int Q>
__host__ __device__ inline void shape_jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = rn_ddiv(rn_dsub(a[Q][Q], a[P][P]), rn_dmul(2.0, apq));
    const double root = rn_dsqrt(rn_dadd(rn_dmul(theta, theta), 1.0));
    const double t = theta >= 0.0 ? rn_ddiv(1.0, rn_dadd(theta, root)) : rn_ddiv(-1.0, rn_dsub(root, theta));
    const double cs = rn_ddiv(1.0, rn_dsqrt(rn_dadd(rn_dmul(t, t), 1.0)));
    const double sn = rn_dmul(t, cs);
    const double h = rn_dmul(t, apq);
    a[P][P] = rn_dsub(a[P][P], h);
    a[Q][Q] = rn_dadd(a[Q][Q], h);
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = rn_dsub(rn_dmul(cs, arp), rn_dmul(sn, arq));
    a[R][Q] = a[Q][R] = rn_dadd(rn_dmul(sn, arp), rn_dmul(cs, arq));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = rn_dsub(rn_dmul(cs, vkp), rn_dmul(sn, vkq));
        v[k][Q] = rn_dadd(rn_dmul(sn, vkp), rn_dmul(cs, vkq));
    }
}

// stable descending order: the later of two neighbours moves up only when it is strictly larger
template <int I, int J>
__host__ __device__ inline void shape_order(double (&d)[3], double (&v)[3][3]) {
    if (d[J] > d[I]) {
        const double t = d[I]; d[I] = d[J]; d[J] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double u = v[k][I]; v[k][I] = v[k][J]; v[k][J] = u; }
    }
}

// steps 1b and 2: S = the sums of x, y, z, xx, xy, xz, yy, yz, zz (fixq(., 32), int64), n >= 3 -> mean, axes, var of *out
__host__ __device__ inline void shape_solve(const long long S[9], int n, ShapeFrame* out) {
    const double fn = (double)n, scale = 1.0 / 4294967296.0;
    double m[3], e[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = rn_ddiv(rn_dmul(rn_ll2d(S[k]), scale), fn);
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = rn_ddiv(rn_dmul(rn_ll2d(S[3 + k]), scale), fn);
    double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    a[0][0] = rn_dsub(e[0], rn_dmul(m[0], m[0]));
    a[0][1] = a[1][0] = rn_dsub(e[1], rn_dmul(m[0], m[1]));
    a[0][2] = a[2][0] = rn_dsub(e[2], rn_dmul(m[0], m[2]));
    a[1][1] = rn_dsub(e[3], rn_dmul(m[1], m[1]));
    a[1][2] = a[2][1] = rn_dsub(e[4], rn_dmul(m[1], m[2]));
    a[2][2] = rn_dsub(e[5], rn_dmul(m[2], m[2]));
#pragma unroll 1
    for (int sweep = 0; sweep < SHAPE_SWEEPS; ++sweep) {
        shape_jacobi_rotate<0, 1>(a, v);
        shape_jacobi_rotate<0, 2>(a, v);
        shape_jacobi_rotate<1, 2>(a, v);
    }
    double d[3] = {a[0][0], a[1][1], a[2][2]};
    shape_order<0, 1>(d, v);
    shape_order<1, 2>(d, v);
    shape_order<0, 1>(d, v);
    const double det = rn_dadd(rn_dsub(rn_dmul(v[0][0], rn_dsub(rn_dmul(v[1][1], v[2][2]), rn_dmul(v[1][2], v[2][1]))),
                                           rn_dmul(v[0][1], rn_dsub(rn_dmul(v[1][0], v[2][2]), rn_dmul(v[1][2], v[2][0])))),
                                 rn_dmul(v[0][2], rn_dsub(rn_dmul(v[1][0], v[2][1]), rn_dmul(v[1][1], v[2][0]))));
    if (det < 0.0) { v[0][2] = -v[0][2]; v[1][2] = -v[1][2]; v[2][2] = -v[2][2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out->mean[k] = m[k];
        out->var[k] = d[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) out->axes[3 * k + j] = v[k][j];
    }
}

// step 3 for one point: q[a] = ((A[0][a] dx + A[1][a] dy) + A[2][a] dz)
__host__ __device__ inline void shape_project(const double* mean, const double* A, float x, float y, float z, double q[3]) {
    const double dx = rn_dsub((double)x, mean[0]), dy = rn_dsub((double)y, mean[1]), dz = rn_dsub((double)z, mean[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        q[a] = rn_dadd(rn_dadd(rn_dmul(A[a], dx), rn_dmul(A[3 + a], dy)), rn_dmul(A[6 + a], dz));
}

// a refused or too small set: its count and status, every other field zero
__host__ __device__ inline void shape_empty(int n, int status, ShapeFrame* out) {
    out->n = n;
    out->status = status;
#pragma unroll
    for (int k = 0; k < 3; ++k) out->mean[k] = out->var[k] = out->lo[k] = out->hi[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) out->axes[k] = 0.0;
}

__host__ __device__ inline bool shape_finite_f(float f) { return fabsf(f) <= 3.402823466e+38f; }   // (false for a NaN)

// step 5: G (row-major 4x4 float32, scene -> template) from a cluster record c and a template record t.  Returns the index of
// the chosen flip, or -1 with G = identity (a status != OK on either side, or a non-finite result).
__host__ __device__ inline int shape_guess(const ShapeFrame& c, const ShapeFrame& t, float G[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = (k % 5 == 0) ? 1.f : 0.f;
    if (c.status != SHAPE_OK || t.status != SHAPE_OK) return -1;
    // the rule's order of operations: score = ((F0 s0) w0 + (F1 s1) w1) + (F2 s2) w2
    double sigma[3], w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = rn_dadd(t.lo[a], t.hi[a]);
        sigma[a] = fabs(s) <= rn_dmul(1.0 / 1048576.0, rn_dsub(t.hi[a], t.lo[a])) ? 0.0 : (-s > 0.0 ? 1.0 : -1.0);
        w[a] = -rn_dadd(rn_dadd(rn_dmul(c.axes[a], c.mean[0]), rn_dmul(c.axes[3 + a], c.mean[1])), rn_dmul(c.axes[6 + a], c.mean[2]));
    }
    const double F[4][3] = {{1.0, 1.0, 1.0}, {1.0, -1.0, -1.0}, {-1.0, 1.0, -1.0}, {-1.0, -1.0, 1.0}};
    double best = 0.0;
    int flip = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double sc = rn_dadd(rn_dadd(rn_dmul(rn_dmul(F[k][0], sigma[0]), w[0]), rn_dmul(rn_dmul(F[k][1], sigma[1]), w[1])),
                                    rn_dmul(rn_dmul(F[k][2], sigma[2]), w[2]));
        if (k == 0 || sc > best) { best = sc; flip = k; }
    }
    const double f0 = flip >= 2 ? -1.0 : 1.0, f1 = (flip == 1 || flip == 3) ? -1.0 : 1.0, f2 = (flip == 1 || flip == 2) ? -1.0 : 1.0;
    float g[12];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double R[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[j] = rn_dadd(rn_dadd(rn_dmul(rn_dmul(t.axes[3 * i], f0), c.axes[3 * j]), rn_dmul(rn_dmul(t.axes[3 * i + 1], f1), c.axes[3 * j + 1])),
                             rn_dmul(rn_dmul(t.axes[3 * i + 2], f2), c.axes[3 * j + 2]));
        const double gi = rn_dsub(t.mean[i], rn_dadd(rn_dadd(rn_dmul(R[0], c.mean[0]), rn_dmul(R[1], c.mean[1])), rn_dmul(R[2], c.mean[2])));
#pragma unroll
        for (int j = 0; j < 3; ++j) { g[4 * i + j] = (float)R[j]; finite = finite && shape_finite_f(g[4 * i + j]); }
        g[4 * i + 3] = (float)gi;
        finite = finite && shape_finite_f(g[4 * i + 3]);
    }
    if (!finite) return -1;
#pragma unroll
    for (int k = 0; k < 12; ++k) G[k] = g[k];
    return flip;
}

}  // namespace cd
