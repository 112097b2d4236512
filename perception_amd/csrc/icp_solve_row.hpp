// icp_solve_row.hpp - icp_step (icp_solve.hpp) executed by a ROW of 16 lanes instead of one: the same IcpState fields, the same
// return value, every rounded operation and its association those of icp_step, so the results are the same bits.  k_icp_lat's
// solve phase calls it (one row per slot); the single-lane icp_step stays the reference and what every other driver calls.
//
// The code is written once against a small "row" abstraction, R:
//   R::V<T>            a value that differs from lane to lane;  x(l) is lane l's copy
//   row.each(f)        runs f(l) for the lanes of the row (device: once, l = the own lane; host check: a loop over 16 lanes)
//   row.read(x, src)   lane src's copy of x (src may differ per lane).  x must have been written in an EARLIER each() block
// Everything outside an each() block is "replicated": computed from read() results and replicated values only, so every lane
// of the row holds the same bits and takes the same branches (rows of one wave may diverge from each other).  The device
// maps read() to ds_bpermute_b32 inside the row (RowLanes below); icp_solve_row_check.cpp maps it to arrays and compares
// every output bit with icp_step on the host, before anything runs on a GPU.
//
// Layout inside a row: lane i holds moment sum i; sigma entry (a, b) is born on lane 6 + 3a + b; row r of U lives on lane r,
// row r of V on lane 4 + r (apply_right touches two columns of every row: lane-local); entry (i, j) of T, R and Tfinal on lane
// 4i + j.  The Jacobi rotation parameters are a serial chain and stay replicated.
#pragma once
#include "icp_solve.hpp"

namespace cd {

#ifndef CD_ROW_SQRT_GE1
#define CD_ROW_SQRT_GE1 1
#endif
#ifndef CD_ROW_RCP_GE1
#define CD_ROW_RCP_GE1 1
#endif

// ---- exact shorter forms of operations whose operand range is known ------------------------------------------------------------
// sqrt_ge1(x) == sqrtf(x) for x in [1, +inf]: the hardware square root (1 ulp) followed by the two-sided one-ulp correction the
// compiler's IEEE sequence ends with - s-1ulp if (s-1ulp) * s >= x, s+1ulp if (s+1ulp) * s < x, both residuals exact in one fma -
// without that sequence's scaling of denormal inputs and its class test for 0 / inf.  (+inf stays +inf: both residuals are NaN.)
// rcp_ge1(x) == 1.0f / x for 1 <= |x| < 2^126 (a normal result: no scaling needed): the hardware reciprocal (1 ulp), one Newton
// step, and a last step from the exactly computed residual 1 - x * r - the core of the compiler's division without v_div_scale /
// v_div_fmas / v_div_fixup.  Beyond 2^126 the result is denormal and the hardware reciprocal flushes it: NOT valid there.
// Neither equality is argued: cd_icp_solve_batch compares every float of the two domains on the device (1.07e9 and 2.1e9
// values, tests/test_gpu_icp_solve_row.py).  The caller (row_rotation) keeps the arguments inside the domains or discards the
// results.  On the host, and with -DCD_ROW_SQRT_GE1=0 / -DCD_ROW_RCP_GE1=0, they are the plain operations; the host check defines
// CD_ROW_POISON, which makes them return a wrong value outside their domains: a result used from there shows as a difference.
constexpr float RCP_GE1_END = 0x1p126f;
__device__ __forceinline__ float sqrt_ge1(float x) {
#if defined(__HIP_DEVICE_COMPILE__) && CD_ROW_SQRT_GE1
    float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
    const float ed = __builtin_fmaf(-sd, s, x), eu = __builtin_fmaf(-su, s, x);
    s = ed <= 0.f ? sd : s;
    s = eu > 0.f ? su : s;
    return s;
#else
#ifdef CD_ROW_POISON
    if (x < 1.0f) return 12345.f;   // (a NaN stays a NaN, as on the device)
#endif
    return sqrtf(x);
#endif
}
__device__ __forceinline__ float rcp_ge1(float x) {
#if defined(__HIP_DEVICE_COMPILE__) && CD_ROW_RCP_GE1
    float r = __builtin_amdgcn_rcpf(x);
    r = __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
    r = __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
    return r;
#else
#ifdef CD_ROW_POISON
    if (fabsf(x) < 1.0f || fabsf(x) >= RCP_GE1_END) return 12345.f;
#endif
    return 1.0f / x;
#endif
}
// The serial part of one two-sided Jacobi rotation - rot1 and j_right = make_jacobi(n00, n01, n11) of jacobi_svd3 - from the 2x2
// block (m00 m01; m10 m11), bit for bit, in two forms:
//  * short: the square roots (all of 1 + v*v >= 1) and reciprocals (of sqrt(1 + v*v) >= 1 and of tau +- w, |.| >= w >= 1) in the
//    forms above, and r.s = -sign_t * (y / |y|) * |t| * n as (+-|t|) * n: for finite y != 0 the quotient is exactly +-1, so
//    ((-sign_t) * (+-1)) * |t| is |t| with the sign (t > 0) xor (y < 0) - exact, a zero keeps that sign - and the product with n
//    is the original's single rounding;
//  * plain: the statements of jacobi_svd3 and make_jacobi themselves.
// The short form is computed first and kept iff the two reciprocal arguments that can leave [1, 2^126) did not (s1 =
// sqrt(1 + u*u) with u = d / t unbounded, and tau +- w) and y is finite: ONE test per rotation.  It fails for every NaN (a NaN
// anywhere reaches one of the two arguments) and for +-inf; the third reciprocal's argument sqrt(1 + t*t) has |t| <= 1 whenever
// tau +- w passed.  Everything else is recomputed in the plain form (NaN signs and payloads are not worth an argument).
__device__ __forceinline__ void row_rotation(float m00, float m01, float m10, float m11, Rot& rot1, Rot& j_right) {
    const float t = m00 + m11, d = m10 - m01;
    float s1 = 1.0f, x3 = 1.0f, y = 1.0f;
    if (t == 0.f) {
        rot1.c = 0.f;
        rot1.s = d > 0.f ? 1.f : -1.f;
    } else {
        const float u = d / t;
        s1 = sqrt_ge1(1.0f + u * u);
        rot1.c = rcp_ge1(s1);
        rot1.s = rot1.c * u;
    }
    {
        const float n00 = rot1.c * m00 + rot1.s * m10, n01 = rot1.c * m01 + rot1.s * m11;
        const float n11 = -rot1.s * m01 + rot1.c * m11;
        if (n01 == 0.f) {
            j_right = {1.f, 0.f};
        } else {
            y = n01;
            const float tau = (n00 - n11) / (2.0f * fabsf(y));
            const float w = sqrt_ge1(tau * tau + 1.0f);
            x3 = tau > 0.f ? tau + w : tau - w;
            const float tt = rcp_ge1(x3);
            const float n = rcp_ge1(sqrt_ge1(tt * tt + 1.0f));
            const float at = fabsf(tt);
            j_right.s = ((tt > 0.f) != (y < 0.f) ? -at : at) * n;
            j_right.c = n;
        }
    }
    if (!(s1 < RCP_GE1_END && fabsf(x3) < RCP_GE1_END && fabsf(y) < __builtin_inff())) {   // plain form
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
        j_right = make_jacobi(n00, n01, n11);
    }
}

template <int N> struct RowIdx { static constexpr int value = N; };

// icp_step<BOUNDED> on a row.  a(l): moment sum l of the step's n correspondences (lane l holds sum l).  Returns done in every
// lane of the row; so is written by the lanes that own each field.
template <bool BOUNDED, class R>
__device__ __forceinline__ int icp_step_row(R& row, IcpState& so, const typename R::template V<unsigned long long>& a, int n, const IcpParams& prm) {
    using VF = typename R::template V<float>;
    using VD = typename R::template V<double>;
    if (BOUNDED && n < ICP_MIN_CORR) {   // icp_stop_few
        row.each([&](int l) {
            so.T[l] = (l % 5 == 0) ? 1.f : 0.f;
            if (l == 0) so.converged = 0;
        });
        return 1;
    }
    // ---- the 16 means: ONE double division instead of 16 (lanes 0..2 mp, 3..5 mq, 6..14 E[q_a p_b], 15 the MSE) ----
    VD m;
    VF mf;
    row.each([&](int l) {
        m(l) = unfix(a(l), l == 15 ? FIX_SHIFT_D2 : FIX_SHIFT) / (double)n;
        mf(l) = (float)m(l);
    });
    VF sg;   // lanes 6..14: sigma[a][b]
    row.each([&](int l) {
        const int k = (l >= 6 && l < 15) ? l - 6 : 0, ia = k / 3, ib = k - 3 * ia;
        const double mqa = row.read(m, 3 + ia), mpb = row.read(m, ib);
        sg(l) = (float)(m(l) - mqa * mpb);
    });
    float sigma[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) sigma[i][j] = row.read(sg, 6 + 3 * i + j);
    // ---- jacobi_svd3: W replicated, one row of U / V per lane ----
    const float precision = 2.0f * 1.1920928955078125e-07f;
    const float consider_zero = 2.0f * 1.401298464324817e-45f;
    float scale = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) scale = fmaxf(scale, fabsf(sigma[i][j]));
    if (scale == 0.f) scale = 1.f;
    VF wl;   // lanes 6..14: sigma / scale, ONE float division instead of nine
    row.each([&](int l) { wl(l) = sg(l) / scale; });
    float W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[i][j] = row.read(wl, 6 + 3 * i + j);
    VF X[3];   // lane r: U[r][0..2]; lane 4 + r: V[r][0..2] (the other lanes carry rows nobody reads)
    row.each([&](int l) {
        X[0](l) = (l & 3) == 0 ? 1.f : 0.f;
        X[1](l) = (l & 3) == 1 ? 1.f : 0.f;
        X[2](l) = (l & 3) == 2 ? 1.f : 0.f;
    });
    bool finished = false;
    auto pair = [&](auto P, auto Q) {
        constexpr int p = decltype(P)::value, q = decltype(Q)::value;
        const float thr = fmaxf(consider_zero, precision * fmaxf(fabsf(W[p][p]), fabsf(W[q][q])));
        if (fabsf(W[p][q]) > thr || fabsf(W[q][p]) > thr) {
            finished = false;
            Rot rot1, j_right;
            row_rotation(W[p][p], W[p][q], W[q][p], W[q][q], rot1, j_right);
            const Rot j_left = rot_mul(rot1, rot_T(j_right));
            apply_left(W, p, q, j_left);
            apply_right(W, p, q, j_right);
            const Rot j_u = rot_T(j_left);
            row.each([&](int l) {   // apply_right(U, p, q, rot_T(j_left)) on the U lanes, apply_right(V, p, q, j_right) on the V lanes
                const float c = l < 4 ? j_u.c : j_right.c, s = l < 4 ? j_u.s : j_right.s;
                const float x = X[p](l), y = X[q](l);
                X[p](l) = c * x - s * y;
                X[q](l) = s * x + c * y;
            });
        }
    };
    for (int sweep = 0; sweep < 64 && !finished; ++sweep) {
        finished = true;
        pair(RowIdx<1>(), RowIdx<0>());
        pair(RowIdx<2>(), RowIdx<0>());
        pair(RowIdx<2>(), RowIdx<1>());
    }
    float S[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float av = fabsf(W[i][i]);
        S[i] = av;
        if (av != 0.f) {
            const float f = W[i][i] / av;
            row.each([&](int l) { if (l < 4) X[i](l) *= f; });
        }
    }
    // Eigen's selection sort (see jacobi_svd3): S replicated, a column swap is lane-local for U and V alike
#define CD_ROW_SWAP_COLS(ca, cb)                                                                   \
    {                                                                                              \
        const float t_ = S[ca]; S[ca] = S[cb]; S[cb] = t_;                                         \
        row.each([&](int l) { const float u_ = X[ca](l); X[ca](l) = X[cb](l); X[cb](l) = u_; });   \
    }
    {
        int pos = 0;
        float mxv = S[0];
        if (S[1] > mxv) { mxv = S[1]; pos = 1; }
        if (S[2] > mxv) { mxv = S[2]; pos = 2; }
        if (mxv != 0.f) {
            if (pos == 1) CD_ROW_SWAP_COLS(0, 1)
            else if (pos == 2) CD_ROW_SWAP_COLS(0, 2)
            if (S[2] > S[1]) CD_ROW_SWAP_COLS(1, 2)
        }
    }
#undef CD_ROW_SWAP_COLS
#pragma unroll
    for (int i = 0; i < 3; ++i) S[i] *= scale;
    // ---- umeyama: signs, R on lanes 4i + j, the translation column on lanes 4i + 3 ----
    float sd[3] = {1.f, 1.f, 1.f};
    if (det3(sigma) < 0.f) sd[2] = -1.f;
    int rank = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (!(fabsf(S[i]) <= fabsf(S[0]) * 1e-5f)) ++rank;
    if (rank == 2) {   // (rare: the whole U and V in every lane)
        float Uf[3][3], Vf[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Uf[r][c] = row.read(X[c], r);
                Vf[r][c] = row.read(X[c], 4 + r);
            }
        sd[0] = 1.f; sd[1] = 1.f;
        sd[2] = (det3(Uf) * det3(Vf) > 0.f) ? 1.f : -1.f;
    }
    VF rr;   // lanes 4i + j, i, j < 3: R[i][j]
    row.each([&](int l) {
        const int i = l >> 2, j = l & 3;
        const float u0 = row.read(X[0], i), u1 = row.read(X[1], i), u2 = row.read(X[2], i);
        const float v0 = row.read(X[0], 4 + j), v1 = row.read(X[1], 4 + j), v2 = row.read(X[2], 4 + j);
        rr(l) = ((u0 * sd[0]) * v0 + (u1 * sd[1]) * v1) + (u2 * sd[2]) * v2;
    });
    VF t;    // lane l: T[l]
    row.each([&](int l) {
        const int i = l >> 2, j = l & 3, b = l & 12;
        const float r0 = row.read(rr, b), r1 = row.read(rr, b + 1), r2 = row.read(rr, b + 2);
        const float p0 = row.read(mf, 0), p1 = row.read(mf, 1), p2 = row.read(mf, 2), qi = row.read(mf, 3 + (i < 3 ? i : 0));
        const float tr = qi - ((r0 * p0 + r1 * p1) + r2 * p2);
        t(l) = i == 3 ? (j == 3 ? 1.f : 0.f) : (j == 3 ? tr : rr(l));
    });
    // ---- Tfinal = T * Tfinal: entry (i, j) on lane 4i + j, in mat4_mul's association ----
    VF c;
    row.each([&](int l) {
        const int j = l & 3, b = l & 12;
        const float t0 = row.read(t, b), t1 = row.read(t, b + 1), t2 = row.read(t, b + 2), t3 = row.read(t, b + 3);
        c(l) = ((t0 * so.Tfinal[j] + t1 * so.Tfinal[4 + j]) + t2 * so.Tfinal[8 + j]) + t3 * so.Tfinal[12 + j];
    });
    // ---- DefaultConvergenceCriteria::hasConverged, replicated ----
    const int iters = so.iters + 1;
    int done = 0;
    bool mse_seen = false;
    double mse = 0.0;
    if (iters >= prm.max_iter) {
        done = 1;
    } else {
        const float T0 = row.read(t, 0), T5 = row.read(t, 5), T10 = row.read(t, 10), T3 = row.read(t, 3), T7 = row.read(t, 7), T11 = row.read(t, 11);
        const double cos_angle = 0.5 * (double)(((T0 + T5) + T10) - 1.0f);
        const double translation_sqr = (double)((T3 * T3 + T7 * T7) + T11 * T11);
        if (cos_angle >= prm.rot_thr && translation_sqr <= prm.trans_eps) {
            done = 1;
        } else {
            mse = row.read(m, 15);
            const double prev = so.prev_mse;
            if (fabs(mse - prev) < prm.abs_mse) done = 1;
            else if (fabs(mse - prev) / prev < prm.rel_mse) done = 1;
            mse_seen = true;
        }
    }
    row.each([&](int l) {
        so.Tfinal[l] = c(l);
        so.T[l] = t(l);
        if (l == 0) {
            so.iters = iters;
            if (mse_seen) so.prev_mse = mse;
            so.converged = done;
        }
    });
    return done;
}

#ifdef __HIPCC__
// The row of the device: 16 consecutive lanes of a wave, exchanges through ds_bpermute_b32 (the LDS crossbar; no memory is
// touched).  A row only ever reads its own lanes, which execute together.
struct RowLanes {
    template <class T>
    struct V {
        T v;
        __device__ __forceinline__ T& operator()(int) { return v; }
        __device__ __forceinline__ const T& operator()(int) const { return v; }
    };
    int l, base;   // lane within the row; byte address of the row's first lane for ds_bpermute
    __device__ __forceinline__ explicit RowLanes(int thread) {   // the thread's index in a workgroup of whole waves
        const int lane = thread & 63;
        l = lane & 15;
        base = (lane & 48) << 2;
    }
    template <class F> __device__ __forceinline__ void each(F&& f) { f(l); }
    __device__ __forceinline__ int read_word(int w, int src) const {
#ifdef __HIP_DEVICE_COMPILE__
        return __builtin_amdgcn_ds_bpermute(base + (src << 2), w);
#else
        return w;   // (the host pass of the compiler only parses this)
#endif
    }
    __device__ __forceinline__ float read(const V<float>& x, int src) const { return __int_as_float(read_word(__float_as_int(x.v), src)); }
    __device__ __forceinline__ double read(const V<double>& x, int src) const {
        const long long b = __double_as_longlong(x.v);
        const unsigned lo = (unsigned)read_word((int)(unsigned)b, src), hi = (unsigned)read_word((int)(unsigned)((unsigned long long)b >> 32), src);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
};
#endif

}  // namespace cd
