// verify_math.hpp - canonical rule C14: the box of an ICP pose rendered into the depth image it was found in.
// Shared by the host entries cd_verify_pixel / cd_verify_box_host and the kernel of k_verify.hip, so that all three run the
// same sequence of correctly rounded double operations.  On the device every operation is an explicit round-to-nearest
// intrinsic (no contraction can enter whatever the compile flags); the host build has -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "rn_ops.hpp"

namespace cd {

enum { VERIFY_MISS = 0, VERIFY_AGREE = 1, VERIFY_THROUGH = 2, VERIFY_OCCLUDED = 3, VERIFY_INVALID = 4 };

struct VerifyCam { double fx, fy, cx, cy, depth_scale; int32_t width, height; };   // cd_depth_camera, the floats widened
struct VerifyCounts { int32_t n_hit, n_agree, n_through, n_occluded, n_invalid; unsigned long long agree_abs_um; };

// what is uniform over the pixels of one box: the columns of R, the ray origin in the box frame, the half dimensions
struct VerifySetup {
    double col[3][3];   // col[a][r] = R[r][a]
    double o[3], half[3];
    int32_t verified;   // step 1
};

__host__ __device__ inline bool verify_finite(double v) { return v - v == 0.0; }   // (false for NaN and the infinities)

// steps 1 and 2 (the per-box part)
__host__ __device__ inline void verify_setup(const double* pose, const double* dims, VerifySetup* s) {
    bool ok = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) ok = ok && verify_finite(pose[4 * r + c]);
    const double t0 = pose[3], t1 = pose[7], t2 = pose[11];
    for (int a = 0; a < 3; ++a) {
        s->col[a][0] = pose[a];
        s->col[a][1] = pose[4 + a];
        s->col[a][2] = pose[8 + a];
        s->half[a] = rn_ddiv(dims[a], 2.0);
        s->o[a] = -rn_dadd(rn_dadd(rn_dmul(s->col[a][0], t0), rn_dmul(s->col[a][1], t1)), rn_dmul(s->col[a][2], t2));
    }
    for (int k = 0; k < 8; ++k) {
        const double x = (k & 4) ? s->half[0] : -s->half[0], y = (k & 2) ? s->half[1] : -s->half[1], z = (k & 1) ? s->half[2] : -s->half[2];
        const double zc = rn_dadd(rn_dadd(rn_dadd(rn_dmul(pose[8], x), rn_dmul(pose[9], y)), rn_dmul(pose[10], z)), t2);
        ok = ok && zc > 0.0;
    }
    s->verified = ok ? 1 : 0;
}

// steps 2 and 3 for the ray of pixel (u, v): true when it hits, *z_r the camera z of the entry point
__host__ __device__ inline bool verify_hit(const VerifySetup& s, const VerifyCam& cam, int u, int v, double* z_r) {
    const double dx = rn_ddiv(rn_dsub((double)u, cam.cx), cam.fx), dy = rn_ddiv(rn_dsub((double)v, cam.cy), cam.fy);
    double tn = -INFINITY, tf = INFINITY;
    bool miss = false;
    for (int a = 0; a < 3; ++a) {
        const double dd = rn_dadd(rn_dadd(rn_dmul(s.col[a][0], dx), rn_dmul(s.col[a][1], dy)), s.col[a][2]);
        if (dd == 0.0) {
            miss = miss || fabs(s.o[a]) > s.half[a];
        } else {
            const double t1 = rn_ddiv(rn_dsub(-s.half[a], s.o[a]), dd), t2 = rn_ddiv(rn_dsub(s.half[a], s.o[a]), dd);
            const double lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
            tn = lo > tn ? lo : tn;
            tf = hi < tf ? hi : tf;
        }
    }
    *z_r = tn;
    return !miss && tn <= tf && tn > 0.0;
}

// step 4 for a hit pixel; *um: the pixel's term of agree_abs_um (AGREE only; terms of 2^63 and over count as 2^63 - 1)
__host__ __device__ inline int verify_class(double z_r, uint16_t d, double depth_scale, double tau, unsigned long long* um) {
    if (d == 0) return VERIFY_INVALID;
    const double z_m = rn_dmul((double)d, depth_scale);
    if (rn_dsub(z_m, z_r) > tau) return VERIFY_THROUGH;
    if (rn_dsub(z_r, z_m) > tau) return VERIFY_OCCLUDED;
    const double e = rn_dadd(rn_dmul(fabs(rn_dsub(z_m, z_r)), 1e6), 0.5);
    *um = e < 9223372036854775808.0 ? (unsigned long long)(long long)e : 9223372036854775807ull;
    return VERIFY_AGREE;
}

// the per-pixel function: steps 2-4, and the pixel's contribution to the counts of step 5
__host__ __device__ inline int verify_pixel(const VerifySetup& s, const VerifyCam& cam, double tau, int u, int v, uint16_t d, double* z_r,
                                            VerifyCounts* acc) {
    if (!verify_hit(s, cam, u, v, z_r)) return VERIFY_MISS;
    unsigned long long um = 0ull;
    const int cls = verify_class(*z_r, d, cam.depth_scale, tau, &um);
    acc->n_hit += 1;
    acc->n_agree += cls == VERIFY_AGREE;
    acc->n_through += cls == VERIFY_THROUGH;
    acc->n_occluded += cls == VERIFY_OCCLUDED;
    acc->n_invalid += cls == VERIFY_INVALID;
    acc->agree_abs_um += um;
    return cls;
}

// Step 6: a pixel rectangle [x0, x1] x [y0, y1] (empty when x0 > x1 or y0 > y1) outside which every pixel of a verified box is a
// miss.  The rendered solid is S = { t + p : |R^T p| <= half }.  With A = R^T R = I + E and |E_ij| <= eps, S = { t + R q :
// |A q| <= half }, and |A q| <= half puts every |q_i| within half_i + 3 eps / (1 - 3 eps) * max(half): for eps <= 1e-3 that is
// the box widened by less than 0.4 % of its largest half dimension - the rectangle is taken around the projected corners of the
// box widened by 1 %, then by one pixel, and clipped to the image.  A pinhole maps the hull of points in front of the camera
// to the hull of their images, so the corners' bounding rectangle bounds the silhouette.  Everything else - an R that is not
// orthonormal to 1e-3, a widened corner that is not in front of the camera, a projection that is not a number - gets the
// whole image, which needs no proof.  Every value is clamped as a double before it becomes an int.
__host__ __device__ inline void verify_rect(const VerifySetup& s, const double* pose, const VerifyCam& cam, int32_t* x0, int32_t* y0,
                                            int32_t* x1, int32_t* y1) {
    *x0 = 0; *y0 = 0; *x1 = cam.width - 1; *y1 = cam.height - 1;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double g = s.col[a][0] * s.col[b][0] + s.col[a][1] * s.col[b][1] + s.col[a][2] * s.col[b][2] - (a == b ? 1.0 : 0.0);
            if (!(fabs(g) <= 1e-3)) return;
        }
    const double hm = fmax(s.half[0], fmax(s.half[1], s.half[2]));
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const double x = ((k & 4) ? 1.0 : -1.0) * (s.half[0] + 0.01 * hm), y = ((k & 2) ? 1.0 : -1.0) * (s.half[1] + 0.01 * hm),
                     z = ((k & 1) ? 1.0 : -1.0) * (s.half[2] + 0.01 * hm);
        const double xc = pose[0] * x + pose[1] * y + pose[2] * z + pose[3], yc = pose[4] * x + pose[5] * y + pose[6] * z + pose[7],
                     zc = pose[8] * x + pose[9] * y + pose[10] * z + pose[11];
        if (!(zc > 0.0)) return;
        const double pu = cam.fx * (xc / zc) + cam.cx, pv = cam.fy * (yc / zc) + cam.cy;
        if (!verify_finite(pu) || !verify_finite(pv)) return;
        ulo = fmin(ulo, pu); uhi = fmax(uhi, pu);
        vlo = fmin(vlo, pv); vhi = fmax(vhi, pv);
    }
    const double w1 = (double)(cam.width - 1), h1 = (double)(cam.height - 1);
    // (clamped to [-1, side]: an empty rectangle stays empty, and the conversions are exact)
    *x0 = (int32_t)fmin(fmax(floor(ulo) - 1.0, 0.0), w1 + 1.0);
    *x1 = (int32_t)fmax(fmin(ceil(uhi) + 1.0, w1), -1.0);
    *y0 = (int32_t)fmin(fmax(floor(vlo) - 1.0, 0.0), h1 + 1.0);
    *y1 = (int32_t)fmax(fmin(ceil(vhi) + 1.0, h1), -1.0);
}

}  // namespace cd
