// pose_info_math.hpp - the arithmetic of canonical rule C23 (perception_amd/pose_info.py is the specification): the
// pose information of a (cluster, lattice template) pair.  Written once for host and device through rn_ops.hpp: the template's
// centre and length (step 3), the six float32 terms of a kept point (step 4), and - pose_finish - the information matrix from the
// eighteen integer sums, its cyclic Jacobi decomposition, the ordering and the summaries (steps 5 to 9).  k_pose_info.hip runs
// the pass over the points on the GPU and one lane of it runs pose_finish; pose_passes_host below is the pass on the CPU
// (cd_pose_info_host, pose_info_math_check.cpp) with rule C5's neighbour by brute force.  One correctly rounded IEEE operation
// per operator, only + - x / sqrt, integer sums: the record does not depend on who computes it.
//
// The information counts what the template's SURFACES constrain and nothing else: the outline of a partial view adds nothing, and
// hidden faces are not reasoned about.
//
// pose_finish keeps every array it indexes at run time in a caller-given workspace of POSE_WS doubles (LDS on the device: a
// private array indexed by a loop variable would go to scratch memory) and takes the sums through a pointer for the same reason.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "common.hpp"

namespace cd {

constexpr int POSE_AXIS_SUMS = 6;                   // per axis: p_c, p_b, p_c p_c, p_b p_b, p_c p_b at 2^32, r r at 2^36
constexpr int POSE_NSUMS = 3 * POSE_AXIS_SUMS;
constexpr int POSE_RR = 5;                          // index of r r among an axis' sums
constexpr int POSE_SWEEPS = 5;                      // cyclic Jacobi sweeps, fixed (profiles/EXPERIMENTS.md has what they leave)
constexpr int POSE_MAX_POINTS = 1 << 19;            // rule C4's N
constexpr int POSE_MIN_CORR = 3;
constexpr int POSE_WS = 80;                         // doubles of workspace: a[36], v[36], lambda[6], spare
// the range of LatFix: every term of a point below 2^18 at 2^32 and below 2^14 at 2^36
constexpr float POSE_FIX_P_MAX = 512.f, POSE_FIX_R_MAX = 128.f;

__host__ __device__ inline int pose_shift(int j) { return j == POSE_RR ? FIX_SHIFT_D2 : FIX_SHIFT; }

// step 3: the centre and the length of a template (host, at cd_set_template).  xyz: m >= 1 packed triples
inline void pose_box(const float* xyz, int m, float c0[3], double* length) {
    float lo[3] = {xyz[0], xyz[1], xyz[2]}, hi[3] = {xyz[0], xyz[1], xyz[2]};
    for (int j = 1; j < m; ++j)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * (size_t)j + a];
            lo[a] = v < lo[a] ? v : lo[a];
            hi[a] = v > hi[a] ? v : hi[a];
        }
    double e[3];
    for (int a = 0; a < 3; ++a) {
        c0[a] = rn_fmul(rn_fadd(lo[a], hi[a]), 0.5f);
        e[a] = rn_dsub((double)hi[a], (double)lo[a]);
    }
    const double L = rn_dmul(0.5, rn_dsqrt(rn_dadd(rn_dadd(rn_dmul(e[0], e[0]), rn_dmul(e[1], e[1])), rn_dmul(e[2], e[2]))));
    *length = L > 0.0 ? L : 1.0;
}

// step 4: the six terms of a kept point.  A: the aligned point, c0: the centre, w: the constant axis of its neighbour's face, qw:
// the neighbour's coordinate on that axis.  (Selects, not an index: a register array indexed by w would go to scratch memory.)
__host__ __device__ inline void pose_terms(float ax, float ay, float az, float cx, float cy, float cz, int w, float qw, float (&t)[POSE_AXIS_SUMS]) {
    const float px = rn_fsub(ax, cx), py = rn_fsub(ay, cy), pz = rn_fsub(az, cz);
    const float pb = w == 0 ? py : (w == 1 ? pz : px), pc = w == 0 ? pz : (w == 1 ? px : py);
    const float r = rn_fsub(qw, w == 0 ? ax : (w == 1 ? ay : az));
    t[0] = pc;
    t[1] = pb;
    t[2] = rn_fmul(pc, pc);
    t[3] = rn_fmul(pb, pb);
    t[4] = rn_fmul(pc, pb);
    t[5] = rn_fmul(r, r);
}

// rule C4's conversion on the host (the device's fixq)
inline long long pose_fix_host(float v, int shift) { return std::llrint(std::ldexp((double)v, shift)); }

inline bool pose_setting_ok(double max_range, double min_support) {
    return std::isfinite(max_range) && max_range > 0.0 && std::isfinite(min_support) && min_support > 0.0;   // (a NaN fails)
}

__host__ __device__ inline bool pose_finite(float x, float y, float z) {
    uint32_t b[3];
    __builtin_memcpy(&b[0], &x, 4); __builtin_memcpy(&b[1], &y, 4); __builtin_memcpy(&b[2], &z, 4);
    return (b[0] & 0x7f800000u) != 0x7f800000u && (b[1] & 0x7f800000u) != 0x7f800000u && (b[2] & 0x7f800000u) != 0x7f800000u;
}

// a record that holds n_source, the status and zeros (and, where the pass has run, its counts)
__host__ __device__ inline void pose_empty(int n, int status, int n_in, int nf0, int nf1, int nf2, cd_pose_info* out) {
    out->n_source = n; out->n_in = n_in;
    out->n_face[0] = nf0; out->n_face[1] = nf1; out->n_face[2] = nf2;
    out->n_constrained = 0; out->well_posed = 0; out->status = status;
#pragma unroll 1
    for (int k = 0; k < 36; ++k) { out->eigenvectors[k] = 0.0; out->covariance[k] = 0.0; }
#pragma unroll 1
    for (int k = 0; k < 6; ++k) { out->eigenvalues[k] = 0.0; out->weakest[k] = 0.0; }
    out->sigma2 = 0.0;
    out->centre[0] = out->centre[1] = out->centre[2] = 0.0;
    out->length = 0.0;
}

// step 9 as far as it can be told without the points: CD_OK means "run the pass".  m: the slot's points, faces: its lattice faces
inline int pose_pre_status(int m, int faces, const float* T) {
    if (m <= 0) return CD_ERR_NO_TEMPLATE;
    if (faces <= 0) return CD_ERR_INVALID_ARG;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(T[i])) return CD_ERR_INVALID_ARG;
    return CD_OK;
}

// one Jacobi rotation of the pair (p, q) of the symmetric 6 x 6 matrix a (all 36 entries kept) and the rotations so far v:
// shape_jacobi_rotate's sequence of operations for six rows
__host__ __device__ inline void pose_jacobi_rotate(double* a, double* v, int p, int q) {
    const double apq = a[6 * p + q];
    if (apq == 0.0) return;
    const double app = a[7 * p], aqq = a[7 * q];
    const double theta = rn_ddiv(rn_dsub(aqq, app), rn_dmul(2.0, apq));
    const double root = rn_dsqrt(rn_dadd(rn_dmul(theta, theta), 1.0));
    const double t = theta >= 0.0 ? rn_ddiv(1.0, rn_dadd(theta, root)) : rn_ddiv(-1.0, rn_dsub(root, theta));
    const double cs = rn_ddiv(1.0, rn_dsqrt(rn_dadd(rn_dmul(t, t), 1.0)));
    const double sn = rn_dmul(t, cs);
    const double h = rn_dmul(t, apq);
    a[7 * p] = rn_dsub(app, h);
    a[7 * q] = rn_dadd(aqq, h);
    a[6 * p + q] = a[6 * q + p] = 0.0;
#pragma unroll 1
    for (int r = 0; r < 6; ++r) {
        if (r == p || r == q) continue;
        const double arp = a[6 * r + p], arq = a[6 * r + q];
        a[6 * r + p] = a[6 * p + r] = rn_dsub(rn_dmul(cs, arp), rn_dmul(sn, arq));
        a[6 * r + q] = a[6 * q + r] = rn_dadd(rn_dmul(sn, arp), rn_dmul(cs, arq));
    }
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const double vkp = v[6 * k + p], vkq = v[6 * k + q];
        v[6 * k + p] = rn_dsub(rn_dmul(cs, vkp), rn_dmul(sn, vkq));
        v[6 * k + q] = rn_dadd(rn_dmul(sn, vkp), rn_dmul(cs, vkq));
    }
}

// entry k of a permutation of 0 .. 5 packed three bits each
__host__ __device__ inline int pose_perm(unsigned perm, int k) { return (int)((perm >> (3 * k)) & 7u); }

// steps 5 to 9 from what the pass left: n points of which `bad` had a non-finite aligned coordinate, the counts nf0..2 per axis,
// S[POSE_NSUMS] the sums (the constants of LatFix already taken off), the slot's centre and length.  ws: POSE_WS doubles.
__host__ __device__ inline void pose_finish(int n, int bad, int nf0, int nf1, int nf2, const long long* S, float cx, float cy, float cz, double L,
                                            double min_support, int accepted, double* ws, cd_pose_info* out) {
    if (bad != 0) { pose_empty(n, CD_ERR_INVALID_ARG, 0, 0, 0, 0, out); return; }
    const int n_in = nf0 + nf1 + nf2;
    if (n_in < POSE_MIN_CORR) { pose_empty(n, CD_ERR_FEW_CORRESPONDENCES, n_in, nf0, nf1, nf2, out); return; }
    if (n > POSE_MAX_POINTS) { pose_empty(n, CD_ERR_CAPACITY, n_in, nf0, nf1, nf2, out); return; }
    pose_empty(n, CD_OK, n_in, nf0, nf1, nf2, out);
    double *a = ws, *v = ws + 36, *lam = ws + 72;
    const double scale = 1.0 / 4294967296.0;   // 2^-32: the product is exact
    // step 5
#pragma unroll 1
    for (int k = 0; k < 36; ++k) { a[k] = 0.0; v[k] = (k % 7 == 0) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int ax = 0; ax < 3; ++ax) {
        const int b = ax == 2 ? 0 : ax + 1, c = ax == 0 ? 2 : ax - 1;
        const long long* s = S + POSE_AXIS_SUMS * ax;
        const double s_c = rn_dmul(rn_ll2d(s[0]), scale), s_b = rn_dmul(rn_ll2d(s[1]), scale), s_cc = rn_dmul(rn_ll2d(s[2]), scale),
                     s_bb = rn_dmul(rn_ll2d(s[3]), scale), s_cb = rn_dmul(rn_ll2d(s[4]), scale);
        const double cnt = (double)(ax == 0 ? nf0 : (ax == 1 ? nf1 : nf2));
        a[7 * b] = rn_dadd(a[7 * b], rn_ddiv(rn_ddiv(s_cc, L), L));
        a[7 * c] = rn_dadd(a[7 * c], rn_ddiv(rn_ddiv(s_bb, L), L));
        a[6 * b + c] = a[6 * c + b] = rn_dadd(a[6 * b + c], -rn_ddiv(rn_ddiv(s_cb, L), L));
        a[6 * (3 + ax) + b] = a[6 * b + 3 + ax] = rn_dadd(a[6 * (3 + ax) + b], rn_ddiv(s_c, L));
        a[6 * (3 + ax) + c] = a[6 * c + 3 + ax] = rn_dadd(a[6 * (3 + ax) + c], -rn_ddiv(s_b, L));
        a[7 * (3 + ax)] = rn_dadd(a[7 * (3 + ax)], cnt);
    }
    // step 6
#pragma unroll 1
    for (int sweep = 0; sweep < POSE_SWEEPS; ++sweep) {
#pragma unroll 1
        for (int p = 0; p < 5; ++p) {
#pragma unroll 1
            for (int q = p + 1; q < 6; ++q) pose_jacobi_rotate(a, v, p, q);
        }
    }
    // ascending, equal values in index order: a stable insertion sort of the six indices, three bits each in one word
#pragma unroll 1
    for (int k = 0; k < 6; ++k) lam[k] = a[7 * k];
    unsigned perm = 0u;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) perm |= (unsigned)k << (3 * k);
#pragma unroll 1
    for (int i = 1; i < 6; ++i) {
#pragma unroll 1
        for (int j = i; j > 0 && lam[pose_perm(perm, j - 1)] > lam[pose_perm(perm, j)]; --j) {
            const unsigned lo = (unsigned)pose_perm(perm, j - 1), hi = (unsigned)pose_perm(perm, j);
            perm = (perm & ~(63u << (3 * (j - 1)))) | (hi << (3 * (j - 1))) | (lo << (3 * j));
        }
    }
    int n_con = 0;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int col = pose_perm(perm, k);
        const double l = lam[col];
        out->eigenvalues[k] = l;
        if (l >= min_support) ++n_con;
        int big = 0;
        double mag = fabs(v[col]);
#pragma unroll 1
        for (int i = 1; i < 6; ++i) { const double m = fabs(v[6 * i + col]); if (m > mag) { mag = m; big = i; } }
        const bool flip = v[6 * big + col] < 0.0;
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            const double x = flip ? -v[6 * i + col] : v[6 * i + col];
            v[6 * i + col] = x;
            out->eigenvectors[6 * k + i] = x;
            if (k == 0) out->weakest[i] = x;
        }
    }
    // steps 7 and 8
    out->n_constrained = n_con;
    out->well_posed = (accepted && n_con == 6) ? 1 : 0;
    const long long s_rr = (long long)((unsigned long long)S[POSE_RR] + (unsigned long long)S[POSE_AXIS_SUMS + POSE_RR] + (unsigned long long)S[2 * POSE_AXIS_SUMS + POSE_RR]);
    const double sigma2 = rn_ddiv(rn_dmul(rn_ll2d(s_rr), 1.0 / 68719476736.0), (double)n_in);   // 2^-36
    out->sigma2 = sigma2;
    const double inv_L = rn_ddiv(1.0, L);
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
#pragma unroll 1
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
#pragma unroll 1
            for (int k = 0; k < 6; ++k) {
                const int col = pose_perm(perm, k);
                if (lam[col] >= min_support) acc = rn_dadd(acc, rn_ddiv(rn_dmul(v[6 * i + col], v[6 * j + col]), lam[col]));
            }
            out->covariance[6 * i + j] = rn_dmul(rn_dmul(i < 3 ? inv_L : 1.0, rn_dmul(sigma2, acc)), j < 3 ? inv_L : 1.0);
        }
    }
    out->centre[0] = (double)cx; out->centre[1] = (double)cy; out->centre[2] = (double)cz;
    out->length = L;
}

// the constant axis of every template point's face: a lattice's faces follow one another, face f from base[f] (template_prep.hpp)
inline void pose_face_axes(const IcpLattice& L, int m, int* face_w) {
    for (int f = 0; f < L.nface; ++f) {
        const int end = f + 1 < L.nface ? L.base[f + 1] : m;
        for (int j = L.base[f]; j < end && j < m; ++j) face_w[j] = L.w[f];
    }
}

// The pass on the host: rule C5's neighbour by brute force (the lowest index at the least canonical distance).  tpl: m packed
// triples, face_w[j]: the constant axis of point j's face, src: n packed triples.  S: POSE_NSUMS sums, nf: three counts.
inline void pose_passes_host(const float* tpl, int m, const int* face_w, const float* src, int n, const float* T, float tau, const float c0[3],
                             long long* S, int nf[3], int* bad) {
    for (int i = 0; i < POSE_NSUMS; ++i) S[i] = 0;
    nf[0] = nf[1] = nf[2] = 0;
    *bad = 0;
    for (int i = 0; i < n; ++i) {
        const float* p = src + 3 * (size_t)i;
        const float ax = xform_row(T, 0, p[0], p[1], p[2]), ay = xform_row(T, 1, p[0], p[1], p[2]), az = xform_row(T, 2, p[0], p[1], p[2]);
        if (!pose_finite(ax, ay, az)) { *bad += 1; continue; }
        float best = INFINITY;
        int at = 0;
        for (int j = 0; j < m; ++j) {
            const float d = dist2(ax, ay, az, tpl[3 * (size_t)j], tpl[3 * (size_t)j + 1], tpl[3 * (size_t)j + 2]);
            if (d < best) { best = d; at = j; }
        }
        if (!(best <= tau)) continue;
        const int w = face_w[at];
        float t[POSE_AXIS_SUMS];
        pose_terms(ax, ay, az, c0[0], c0[1], c0[2], w, tpl[3 * (size_t)at + w], t);
        for (int j = 0; j < POSE_AXIS_SUMS; ++j)
            S[POSE_AXIS_SUMS * w + j] = (long long)((unsigned long long)S[POSE_AXIS_SUMS * w + j] + (unsigned long long)pose_fix_host(t[j], pose_shift(j)));
        nf[w] += 1;
    }
}

}  // namespace cd
