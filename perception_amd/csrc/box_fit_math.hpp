// box_fit_math.hpp - the arithmetic of canonical rule C24 (perception_amd/box_fit.py is the specification): the box
// fit.  Steps 1 to 3 (the oriented plane, its metric basis, a point's three integers), step 6 of one hull edge and steps 7 to 9
// (the record) written once for host and device; the whole rule as a plain loop for the host.  k_box_fit.hip runs it on the GPU,
// box_fit_math_check.cpp and cd_box_fit_host on the CPU.  One correctly rounded IEEE double operation per operator, no
// contraction; from step 3 on everything is integer until the record, so the result does not depend on who computes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "prism_math.hpp"

namespace cd {

constexpr int BOX_LDS_POINTS = CD_BOX_FIT_LDS_POINTS;   // a cluster's (qh, u, v) k_box_fit keeps in LDS
constexpr double BOX_BAND_MAX = 64.0;
constexpr float BOX_COORD_MAX = 64.0f;
static_assert(sizeof(cd_box_fit) == 8 * 4 + 23 * 8, "cd_box_fit has no padding: the kernel writes every byte");

inline bool box_band_ok(double band) { return std::isfinite(band) && band > 0.0 && band <= BOX_BAND_MAX; }

struct BoxBasis {   // steps 1 and 2
    double nrm[3], dd, eu[3], ev[3];
    int32_t have, pad;
};

// One cluster of a k_box_fit launch: its n points at pts + src_off, floor(band 65536), the record it fills and its frame's basis
struct BoxItem {
    int32_t src_off, n, rec, band_q;
    BoxBasis B;
};

// (nrm_a eu_b) - (nrm_b eu_a) per component
__host__ __device__ inline void box_cross(const double* a, const double* b, double* c) {
    c[0] = rn_dsub(rn_dmul(a[1], b[2]), rn_dmul(a[2], b[1]));
    c[1] = rn_dsub(rn_dmul(a[2], b[0]), rn_dmul(a[0], b[2]));
    c[2] = rn_dsub(rn_dmul(a[0], b[1]), rn_dmul(a[1], b[0]));
}

// have = 0: a non-finite coefficient or a = b = c = 0 (the basis is then zero, and no point is projected with it)
__host__ __device__ inline BoxBasis box_basis(float a, float b, float c, float d) {
    BoxBasis B;
    for (int j = 0; j < 3; ++j) B.nrm[j] = B.eu[j] = B.ev[j] = 0.0;
    B.dd = 0.0; B.pad = 0;
    B.have = (a == a && b == b && c == c && d == d && fabsf(a) <= 3.402823466e38f && fabsf(b) <= 3.402823466e38f && fabsf(c) <= 3.402823466e38f &&
              fabsf(d) <= 3.402823466e38f && (a != 0.0f || b != 0.0f || c != 0.0f)) ? 1 : 0;
    if (!B.have) return B;
    const PrismPlane P = prism_plane(a, b, c, d);
    B.dd = P.dd;
    for (int j = 0; j < 3; ++j) B.nrm[j] = P.n[j];
    const int k0 = 3 - P.k1 - P.k2, k1 = (k0 + 1) % 3;
    double t[3];
    for (int j = 0; j < 3; ++j) t[j] = rn_dsub(j == k1 ? 1.0 : 0.0, rn_dmul(B.nrm[k1], B.nrm[j]));
    const double len = rn_dsqrt(rn_dadd(rn_dadd(rn_dmul(t[0], t[0]), rn_dmul(t[1], t[1])), rn_dmul(t[2], t[2])));
    for (int j = 0; j < 3; ++j) B.eu[j] = rn_ddiv(t[j], len);
    box_cross(B.nrm, B.eu, B.ev);
    return B;
}

// step 10's test of one point: finite and within the range
__host__ __device__ inline bool box_coord_ok(float x, float y, float z) { return fabsf(x) <= BOX_COORD_MAX && fabsf(y) <= BOX_COORD_MAX && fabsf(z) <= BOX_COORD_MAX; }

__host__ __device__ inline double box_dot(const double* e, double x, double y, double z) { return rn_dadd(rn_dadd(rn_dmul(e[0], x), rn_dmul(e[1], y)), rn_dmul(e[2], z)); }

// step 3 of one point
__host__ __device__ inline void box_quantise(const BoxBasis& B, float x, float y, float z, int32_t* qh, int32_t* u, int32_t* v) {
    const double px = (double)x, py = (double)y, pz = (double)z;
    *qh = prism_quantise(rn_dadd(box_dot(B.nrm, px, py, pz), B.dd));
    *u = prism_quantise(box_dot(B.eu, px, py, pz));
    *v = prism_quantise(box_dot(B.ev, px, py, pz));
}

// floor(band 65536): band <= 64, so below 2^23
__host__ __device__ inline int32_t box_band_q(double band) { return (int32_t)floor(rn_dmul(band, 65536.0)); }

// the biased integer whose unsigned order is qh's
__host__ __device__ inline uint32_t box_key(int32_t qh) { return (uint32_t)qh ^ 0x80000000u; }

struct BoxEdge {   // step 6 of one edge
    int64_t w, g, l2, asum, csum;   // asum = amin + amax, csum = cmin + cmax
    double area;
};

// hull: nh >= 3 strict vertices, u and v interleaved.  Coordinates within 2^23 (step 10's range): differences below 2^24, products
// below 2^48, every sum fits int64 and converts to double exactly.
__host__ __device__ inline BoxEdge box_edge(const int32_t* hull, int nh, int i) {
    const int i1 = i + 1 == nh ? 0 : i + 1;
    const int64_t au = hull[2 * i], av = hull[2 * i + 1], eu = (int64_t)hull[2 * i1] - au, ev = (int64_t)hull[2 * i1 + 1] - av;
    int64_t amin = 0, amax = 0, cmin = 0, cmax = 0;   // (P = A gives 0 for both)
    for (int j = 0; j < nh; ++j) {
        const int64_t du = (int64_t)hull[2 * j] - au, dv = (int64_t)hull[2 * j + 1] - av;
        const int64_t al = du * eu + dv * ev, ac = eu * dv - ev * du;
        amin = al < amin ? al : amin; amax = al > amax ? al : amax;
        cmin = ac < cmin ? ac : cmin; cmax = ac > cmax ? ac : cmax;
    }
    BoxEdge E;
    E.w = amax - amin; E.g = cmax - cmin; E.l2 = eu * eu + ev * ev; E.asum = amin + amax; E.csum = cmin + cmax;
    E.area = rn_ddiv(rn_dmul(rn_ll2d(E.w), rn_ll2d(E.g)), rn_ll2d(E.l2));
    return E;
}

// H_i x H_i+1, a term of the shoelace sum
__host__ __device__ inline int64_t box_shoelace_term(const int32_t* hull, int nh, int i) {
    const int i1 = i + 1 == nh ? 0 : i + 1;
    return (int64_t)hull[2 * i] * (int64_t)hull[2 * i1 + 1] - (int64_t)hull[2 * i + 1] * (int64_t)hull[2 * i1];
}

// a record without a fit: the counts reached so far, the status, zeros (match_slot -1)
__host__ __device__ inline void box_empty(int n, int n_top, int hull_vertices, int status, int overflow, cd_box_fit* out) {
    out->n = n; out->n_top = n_top; out->hull_vertices = hull_vertices; out->edge = 0; out->status = status; out->overflow = overflow;
    out->match_slot = -1; out->reserved = 0;
    out->height_ref = 0.0;
    for (int j = 0; j < 3; ++j) out->dims[j] = 0.0;
    for (int j = 0; j < 16; ++j) out->pose[j] = 0.0;
    out->area = 0.0; out->rectangularity = 0.0; out->match_cost = 0.0;
}

// steps 4 (the height), 7, 8 and 9: the record of a cluster whose hull has nh >= 3 vertices and whose edge `edge` won with E
__host__ __device__ inline void box_finish(const BoxBasis& B, int n, int n_top, int32_t href, int64_t qsum, const int32_t* hull, int nh, int edge, const BoxEdge& E,
                                           int64_t shoelace, cd_box_fit* out) {
    const int i1 = edge + 1 == nh ? 0 : edge + 1;
    const int64_t Au = hull[2 * edge], Av = hull[2 * edge + 1], eu = (int64_t)hull[2 * i1] - Au, ev = (int64_t)hull[2 * i1 + 1] - Av;
    const double height = rn_ddiv(rn_ddiv(rn_ll2d(qsum), (double)n_top), 65536.0);
    const double s = rn_dsqrt(rn_ll2d(E.l2));
    const double p = rn_ddiv(rn_ddiv(rn_ll2d(E.w), s), 65536.0), q = rn_ddiv(rn_ddiv(rn_ll2d(E.g), s), 65536.0);
    int64_t au = p >= q ? eu : -ev, av = p >= q ? ev : eu;
    if (au < 0 || (au == 0 && av < 0)) { au = -au; av = -av; }
    const double axu = rn_ddiv(rn_ll2d(au), s), axv = rn_ddiv(rn_ll2d(av), s);
    const double fa = rn_ddiv(rn_ll2d(E.asum), rn_ll2d(2 * E.l2)), fc = rn_ddiv(rn_ll2d(E.csum), rn_ll2d(2 * E.l2));
    const double cu = rn_dadd(rn_dadd(rn_ll2d(Au), rn_dmul(fa, rn_ll2d(eu))), rn_dmul(fc, rn_ll2d(-ev)));
    const double cv = rn_dadd(rn_dadd(rn_ll2d(Av), rn_dmul(fa, rn_ll2d(ev))), rn_dmul(fc, rn_ll2d(eu)));
    const double cus = rn_ddiv(cu, 65536.0), cvs = rn_ddiv(cv, 65536.0);
    const double up = rn_dsub(rn_ddiv(height, 2.0), B.dd);
    double ex[3], ey[3];
    for (int j = 0; j < 3; ++j) ex[j] = rn_dadd(rn_dmul(axu, B.eu[j]), rn_dmul(axv, B.ev[j]));
    box_cross(B.nrm, ex, ey);
    out->n = n; out->n_top = n_top; out->hull_vertices = nh; out->edge = edge; out->status = CD_OK; out->overflow = 0;
    out->match_slot = -1; out->reserved = 0;
    out->height_ref = rn_ddiv((double)href, 65536.0);
    out->dims[0] = p >= q ? p : q; out->dims[1] = p >= q ? q : p; out->dims[2] = height;
    for (int j = 0; j < 3; ++j) {
        out->pose[4 * j] = ex[j]; out->pose[4 * j + 1] = ey[j]; out->pose[4 * j + 2] = B.nrm[j];
        out->pose[4 * j + 3] = rn_dadd(rn_dadd(rn_dmul(cus, B.eu[j]), rn_dmul(cvs, B.ev[j])), rn_dmul(up, B.nrm[j]));
    }
    out->pose[12] = 0.0; out->pose[13] = 0.0; out->pose[14] = 0.0; out->pose[15] = 1.0;
    const double s2 = 4294967296.0;   // 65536^2
    out->area = rn_ddiv(E.area, s2);
    out->rectangularity = rn_ddiv(rn_ddiv(rn_ddiv(rn_ll2d(shoelace), 2.0), s2), out->area);
    out->match_cost = 0.0;
}

// The rule on the host: n points of `stride` bytes (x y z first).  have_plane = 0: a frame without a plane.
inline void box_fit_host(const float* coeff, const void* xyz, size_t stride, int n, double band, int have_plane, cd_box_fit* out) {
    if (n < 3) { box_empty(n, 0, 0, CD_ERR_FEW_CORRESPONDENCES, 0, out); return; }
    std::vector<float> p((size_t)n * 3);
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        std::memcpy(&p[3 * (size_t)i], (const char*)xyz + (size_t)i * stride, 12);
        ok = ok && box_coord_ok(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]);
    }
    if (!ok) { box_empty(n, 0, 0, CD_ERR_INVALID_ARG, 0, out); return; }
    const BoxBasis B = box_basis(coeff[0], coeff[1], coeff[2], coeff[3]);
    if (!have_plane || !B.have) { box_empty(n, 0, 0, CD_ERR_NO_MODEL, 0, out); return; }
    std::vector<int32_t> qh((size_t)n), uv((size_t)n * 2);
    for (int i = 0; i < n; ++i) box_quantise(B, p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], &qh[(size_t)i], &uv[2 * (size_t)i], &uv[2 * (size_t)i + 1]);
    // 4
    std::vector<int32_t> sorted(qh);
    const int k = 1 + n / 64;
    std::nth_element(sorted.begin(), sorted.begin() + (n - k), sorted.end());
    const int32_t href = sorted[(size_t)(n - k)], thr = href - box_band_q(band);
    std::vector<int32_t> top;
    int64_t qsum = 0;
    for (int i = 0; i < n; ++i)
        if (qh[(size_t)i] >= thr) { top.push_back(uv[2 * (size_t)i]); top.push_back(uv[2 * (size_t)i + 1]); qsum += qh[(size_t)i]; }
    const int n_top = (int)(top.size() / 2);
    // 5
    std::vector<int32_t> hull((size_t)PRISM_MAX_HULL * 2);
    const int nh = prism_hull_host(top.data(), n_top, hull.data(), PRISM_MAX_HULL);
    if (nh > PRISM_MAX_HULL) { box_empty(n, n_top, 0, CD_ERR_CAPACITY, 1, out); return; }
    if (nh < 3) { box_empty(n, n_top, nh, CD_ERR_NO_MODEL, 0, out); return; }
    // 6
    BoxEdge best = box_edge(hull.data(), nh, 0);
    int edge = 0;
    int64_t shoelace = box_shoelace_term(hull.data(), nh, 0);
    for (int i = 1; i < nh; ++i) {
        const BoxEdge E = box_edge(hull.data(), nh, i);
        if (E.area < best.area) { best = E; edge = i; }
        shoelace += box_shoelace_term(hull.data(), nh, i);
    }
    box_finish(B, n, n_top, href, qsum, hull.data(), nh, edge, best, shoelace, out);
}

// cd_box_fit_match
inline void box_match(const double* dims, const double (*slot_dims)[3], uint32_t loaded_mask, double tolerance, int32_t* slot, double* cost) {
    int best = -1;
    double c = 0.0;
    for (int s = 0; s < CD_MAX_TEMPLATES; ++s) {
        if (!((loaded_mask >> s) & 1u)) continue;
        const double ls = std::max(slot_dims[s][0], slot_dims[s][1]), ws = std::min(slot_dims[s][0], slot_dims[s][1]);
        const double k = std::max(std::max(std::fabs(dims[0] - ls), std::fabs(dims[1] - ws)), std::fabs(dims[2] - slot_dims[s][2]));
        if (best < 0 || k < c) { best = s; c = k; }
    }
    if (best >= 0 && c > tolerance) best = -1;
    *slot = best; *cost = c;
}

}  // namespace cd
