// icp_solve.hpp - device code shared by the ICP kernels (k_icp.hip, k_icp_cluster.hip, k_icp_pipe.hip, k_icp_lat.hip): TransformationEstimationSVD
// (pcl::umeyama with Eigen's two-sided Jacobi SVD restated in float32) from the 16 fixed-point moment sums, the
// canonical 4x4 x point product, and icp_step - one PCL iteration's state update, the same for every driver.  Reference: pcl::IterativeClosestPoint as called at
// cuboid_detection/src/iterative_closest_point.cpp:170-178 and object_detection/src/object_pose_detection.cpp:220-228.
#pragma once
#include "common.hpp"

namespace cd {

struct Rot { float c, s; };
__device__ __forceinline__ Rot rot_mul(const Rot& a, const Rot& b) { return {a.c * b.c - a.s * b.s, a.c * b.s + a.s * b.c}; }
__device__ __forceinline__ Rot rot_T(const Rot& a) { return {a.c, -a.s}; }
__device__ __forceinline__ void apply_left(float M[3][3], int p, int q, const Rot& j) {
    for (int i = 0; i < 3; ++i) {
        const float x = M[p][i], y = M[q][i];
        M[p][i] = j.c * x + j.s * y;
        M[q][i] = -j.s * x + j.c * y;
    }
}
__device__ __forceinline__ void apply_right(float M[3][3], int p, int q, const Rot& j) {
    for (int i = 0; i < 3; ++i) {
        const float x = M[i][p], y = M[i][q];
        M[i][p] = j.c * x - j.s * y;
        M[i][q] = j.s * x + j.c * y;
    }
}
__device__ __forceinline__ Rot make_jacobi(float x, float y, float z) {
    if (y == 0.f) return {1.f, 0.f};
    const float tau = (x - z) / (2.0f * fabsf(y));
    const float w = sqrtf(tau * tau + 1.0f);
    const float t = tau > 0.f ? 1.0f / (tau + w) : 1.0f / (tau - w);
    const float sign_t = t > 0.f ? 1.0f : -1.0f;
    const float n = 1.0f / sqrtf(t * t + 1.0f);
    Rot r;
    r.s = -sign_t * (y / fabsf(y)) * fabsf(t) * n;
    r.c = n;
    return r;
}
// Eigen 3.2 JacobiSVD<Matrix3f>(ComputeFullU|ComputeFullV): two-sided Jacobi, float32
__device__ inline void jacobi_svd3(const float A[3][3], float U[3][3], float S[3], float V[3][3]) {
    const float precision = 2.0f * 1.1920928955078125e-07f;
    const float consider_zero = 2.0f * 1.401298464324817e-45f;
    float scale = 0.f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) scale = fmaxf(scale, fabsf(A[i][j]));
    if (scale == 0.f) scale = 1.f;
    float W[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            W[i][j] = A[i][j] / scale;
            U[i][j] = V[i][j] = (i == j) ? 1.f : 0.f;
        }
    bool finished = false;
    for (int sweep = 0; sweep < 64 && !finished; ++sweep) {
        finished = true;
        for (int p = 1; p < 3; ++p)
            for (int q = 0; q < p; ++q) {
                const float thr = fmaxf(consider_zero, precision * fmaxf(fabsf(W[p][p]), fabsf(W[q][q])));
                if (fabsf(W[p][q]) > thr || fabsf(W[q][p]) > thr) {
                    finished = false;
                    const float m00 = W[p][p], m01 = W[p][q], m10 = W[q][p], m11 = W[q][q];
                    Rot rot1;
                    const float t = m00 + m11, d = m10 - m01;
                    if (t == 0.f) {
                        rot1.c = 0.f;
                        rot1.s = d > 0.f ? 1.f : -1.f;
                    } else {
                        const float u = d / t;
                        rot1.c = 1.0f / sqrtf(1.0f + u * u);
                        rot1.s = rot1.c * u;
                    }
                    const float n00 = rot1.c * m00 + rot1.s * m10, n01 = rot1.c * m01 + rot1.s * m11;
                    const float n11 = -rot1.s * m01 + rot1.c * m11;
                    const Rot j_right = make_jacobi(n00, n01, n11);
                    const Rot j_left = rot_mul(rot1, rot_T(j_right));
                    apply_left(W, p, q, j_left);
                    apply_right(U, p, q, rot_T(j_left));
                    apply_right(W, p, q, j_right);
                    apply_right(V, p, q, j_right);
                }
            }
    }
    for (int i = 0; i < 3; ++i) {
        const float a = fabsf(W[i][i]);
        S[i] = a;
        if (a != 0.f) {
            const float f = W[i][i] / a;
            for (int r = 0; r < 3; ++r) U[r][i] *= f;
        }
    }
    // Eigen's selection sort of the singular values (first maximum of S[i..2] goes to i; stops at a zero maximum), written out
    // with constant indices: a run-time column index would put U, V and S into scratch memory (three dependent round trips
    // per solve)
#define CD_SWAP_COLS(a, b)                                                  \
    {                                                                       \
        float t_ = S[a]; S[a] = S[b]; S[b] = t_;                            \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) {                     \
            t_ = U[r][a]; U[r][a] = U[r][b]; U[r][b] = t_;                  \
            t_ = V[r][a]; V[r][a] = V[r][b]; V[r][b] = t_;                  \
        }                                                                   \
    }
    {
        int pos = 0;
        float mxv = S[0];
        if (S[1] > mxv) { mxv = S[1]; pos = 1; }
        if (S[2] > mxv) { mxv = S[2]; pos = 2; }
        if (mxv != 0.f) {
            if (pos == 1) CD_SWAP_COLS(0, 1)
            else if (pos == 2) CD_SWAP_COLS(0, 2)
            if (S[2] > S[1]) CD_SWAP_COLS(1, 2)   // (a zero maximum here means S[1] == S[2] == 0: nothing to swap either way)
        }
    }
#undef CD_SWAP_COLS
    for (int i = 0; i < 3; ++i) S[i] *= scale;
}
__device__ __forceinline__ float det3(const float m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
__device__ __forceinline__ double unfix(unsigned long long s, int shift) { return ldexp((double)(long long)s, -shift); }

// pcl::umeyama(src, dst, false) from the fixed-point moments.  A: [0..2] sum p, [3..5] sum q,
// [6..14] sum q_a p_b, [15] sum d2.
__device__ inline void umeyama_from_moments(const unsigned long long* A, int n, float T[16]) {
    double mp[3], mq[3];
    for (int a = 0; a < 3; ++a) {
        mp[a] = unfix(A[a], FIX_SHIFT) / (double)n;
        mq[a] = unfix(A[3 + a], FIX_SHIFT) / (double)n;
    }
    float sigma[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) sigma[a][b] = (float)(unfix(A[6 + 3 * a + b], FIX_SHIFT) / (double)n - mq[a] * mp[b]);
    float U[3][3], S[3], V[3][3];
    jacobi_svd3(sigma, U, S, V);
    float sd[3] = {1.f, 1.f, 1.f};
    if (det3(sigma) < 0.f) sd[2] = -1.f;
    int rank = 0;
    for (int i = 0; i < 3; ++i)
        if (!(fabsf(S[i]) <= fabsf(S[0]) * 1e-5f)) ++rank;
    if (rank == 2) {
        sd[0] = 1.f; sd[1] = 1.f;
        sd[2] = (det3(U) * det3(V) > 0.f) ? 1.f : -1.f;
    }
    float R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i][j] = ((U[i][0] * sd[0]) * V[j][0] + (U[i][1] * sd[1]) * V[j][1]) + (U[i][2] * sd[2]) * V[j][2];
    const float mpf[3] = {(float)mp[0], (float)mp[1], (float)mp[2]};
    const float mqf[3] = {(float)mq[0], (float)mq[1], (float)mq[2]};
    for (int i = 0; i < 16; ++i) T[i] = 0.f;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[i][j];
        T[4 * i + 3] = mqf[i] - ((R[i][0] * mpf[0] + R[i][1] * mpf[1]) + R[i][2] * mpf[2]);
    }
    T[15] = 1.f;
}

// Rule C8 (cd_set_icp_max_correspondence_distance): the BOUNDED instantiations of the ICP kernels keep a correspondence iff its
// float d2 <= IcpParams::d2_max and count the kept ones next to the moment sums; the solve then divides by that count.  Fewer
// than three is PCL's "Not enough correspondences": the ICP stops BEFORE this iteration's update - Tfinal and iters stay,
// converged = 0 - and T becomes the identity, so that the in-place X <- T X that follows leaves the points where they are.
// (ICP_MIN_CORR and the predicate icp_in_k0: common.hpp)
__device__ __forceinline__ void icp_stop_few(IcpState& so) {
    for (int i = 0; i < 16; ++i) so.T[i] = (i % 5 == 0) ? 1.f : 0.f;
    so.converged = 0;
}

__device__ __forceinline__ void xform(const float* T, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}
// C = A * B of row-major 4x4 matrices, each entry in the association of xform; C must not overlap A or B
__device__ __forceinline__ void mat4_mul(const float* A, const float* B, float* C) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
}

// ONE PCL iteration's state update from the 16 moment sums A of its n correspondences - the single implementation every ICP
// driver calls (k_icp_solve, k_icp_persist, k_icp_cluster, k_icp_pipe / k_icp_pipe_big, k_icp_lat), on one lane:
//   TransformationEstimationSVD (umeyama_from_moments), final_transformation_ = transformation_ * final_transformation_,
//   DefaultConvergenceCriteria::hasConverged in its order: iteration limit, rotation / translation epsilon, absolute MSE,
//   relative MSE (prev_mse moves only when the MSE tests are reached).
// BOUNDED (rule C8): n = the kept correspondences; fewer than three stop the ICP before the update (icp_stop_few).
// Returns done and leaves it in so.converged; so.done and every other bookkeeping stay with the caller.
// icp_step is its ESTIMATE (T from the sums) followed by icp_step_tail: everything after the estimate, given T, the d2 sum
// and n.  The plane-weighted step of rule C17 (k_icp_plane.hip) has an estimate of its own and calls the same tail.
__device__ __forceinline__ int icp_step_tail(IcpState& so, const float* T, unsigned long long sum_d2, int n, const IcpParams& prm) {
    float Tf[16];
    mat4_mul(T, so.Tfinal, Tf);
    for (int i = 0; i < 16; ++i) so.Tfinal[i] = Tf[i];
    so.iters += 1;
    int done = 0;
    if (so.iters >= prm.max_iter) {
        done = 1;
    } else {
        const double cos_angle = 0.5 * (double)(((T[0] + T[5]) + T[10]) - 1.0f);
        const double translation_sqr = (double)((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]);
        if (cos_angle >= prm.rot_thr && translation_sqr <= prm.trans_eps) {
            done = 1;
        } else {
            const double mse = unfix(sum_d2, FIX_SHIFT_D2) / (double)n;
            if (fabs(mse - so.prev_mse) < prm.abs_mse) done = 1;
            else if (fabs(mse - so.prev_mse) / so.prev_mse < prm.rel_mse) done = 1;
            so.prev_mse = mse;
        }
    }
    for (int i = 0; i < 16; ++i) so.T[i] = T[i];
    so.converged = done;
    return done;
}
template <bool BOUNDED>
__device__ __forceinline__ int icp_step(IcpState& so, const unsigned long long* A, int n, const IcpParams& prm) {
    if (BOUNDED && n < ICP_MIN_CORR) { icp_stop_few(so); return 1; }
    float T[16];
    umeyama_from_moments(A, n, T);
    return icp_step_tail(so, T, A[15], n, prm);
}

// The 16 fixed-point moment terms of ONE correspondence (rule C4): S[0..2] p, [3..5] q, [6..14] q_a p_b, [15] d2.
// FAST: the conversion is fixq_fast (the caller has checked its range condition) instead of fixq - the same integers.
template <bool FAST = false>
__device__ __forceinline__ void moment_terms(const float (&pv)[3], const float (&qv)[3], float d2, unsigned long long (&S)[16]) {
    auto fix = [](float v, int shift) { return FAST ? fixq_fast(v, shift) : (unsigned long long)fixq(v, shift); };
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        S[a] = fix(pv[a], FIX_SHIFT);
        S[3 + a] = fix(qv[a], FIX_SHIFT);
#pragma unroll
        for (int b = 0; b < 3; ++b) S[6 + 3 * a + b] = fix(__fmul_rn(qv[a], pv[b]), FIX_SHIFT);
    }
    S[15] = fix(d2, FIX_SHIFT_D2);
}

}  // namespace cd
