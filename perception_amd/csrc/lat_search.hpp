// lat_search.hpp - device code shared by the kernels that register clouds against LATTICE templates (k_icp_lat.hip,
// k_icp_plane.hip, k_pose_info.hip, and k_lat_nn): the face descriptors and the one table staging (lat_stage_tables), the
// closed-form nearest neighbour of a query (lat_nearest, lat_nearest_axes, the tie walk; lat_nearest_any picks among them),
// the raw-bits form of rule C4's conversion with its general side path (LatFix, lat_fix_terms, lat_fix_d2, lat_fix_offset),
// the pass loop over a cluster's points (lat_for_passes) and the final transform + getFitnessScore pass (lat_fitness_pass).
// The search is derived and measured in k_icp_lat.hip's header comment.  (k_icp_lat keeps its own text of the staging, the
// dispatch, the accumulate and the two loops - the comment above its LatSlot says why: what is mended here is mended there.)
#pragma once
#include "kernels.hpp"
#include "icp_solve.hpp"

namespace cd {

// face descriptors: what the per-query face loop needs as wave-uniform values (scalar registers after unrolling with constant
// indices) - the constant coordinate and two all-ones / all-zeros words that say which axis it replaces - the rest as LDS
// words read per lane after the loop (s_face[f] = constant axis, fast axis, first index, constant coordinate)
struct LatFaces {
    int nface;
    unsigned m0[LAT_MAX_FACES], m1[LAT_MAX_FACES], m2[LAT_MAX_FACES];   // ~0 when the face's constant axis is x / y / z
    float c[LAT_MAX_FACES];
    int nx, ny, nz, tox, toy, toz;   // entries and first entry of the axis tables (separate scalars: an array indexed by a face's axis would be put into scratch memory)
    float ox, oy, oz, ivx, ivy, ivz;   // (ox = -X[0] / step, ivx = 1 / step: IcpLattice::noi, inv)
    int axes;                          // IcpLattice::axes_distinct: one face per axis at the most - lat_nearest_axes applies
    int afx, afy, afz;                 // the face of constant x / y / z (-1: none)
    float cax, cay, caz;               // its constant coordinate (NaN: none)
};

// the face words of a template as wave-uniform values (scalar loads)
__device__ __forceinline__ void lat_faces_load(const IcpLattice* __restrict__ L, LatFaces& F) {
    F.nface = L->nface;
#pragma unroll
    for (int f = 0; f < LAT_MAX_FACES; ++f) { F.m0[f] = L->m0[f]; F.m1[f] = L->m1[f]; F.m2[f] = L->m2[f]; F.c[f] = L->c[f]; }
    F.nx = L->n[0]; F.ny = L->n[1]; F.nz = L->n[2]; F.tox = L->toff[0]; F.toy = L->toff[1]; F.toz = L->toff[2];
    F.ox = L->noi[0]; F.oy = L->noi[1]; F.oz = L->noi[2]; F.ivx = L->inv[0]; F.ivy = L->inv[1]; F.ivz = L->inv[2];
    F.axes = L->axes_distinct;
    F.afx = L->axis_face[0]; F.afy = L->axis_face[1]; F.afz = L->axis_face[2];
    // (in vector registers from here on: a v_cndmask whose condition is a scalar mask has no room for a second scalar
    // operand, and the compiler would move each constant into a register again in every pass)
    asm("v_mov_b32 %0, %1" : "=v"(F.cax) : "s"(L->axis_c[0]));
    asm("v_mov_b32 %0, %1" : "=v"(F.cay) : "s"(L->axis_c[1]));
    asm("v_mov_b32 %0, %1" : "=v"(F.caz) : "s"(L->axis_c[2]));
}

// The ntab entries of a template's axis tables and its two rows of face words into LDS, by a group of `step` threads of which
// the caller is thread t.  No barrier inside: the caller's follows.  (ntab = L->ntab <= LAT_MAX_TAB: lattice_tables refuses a
// template whose tables do not fit, and the device's IcpLattice records are only ever copies of lattice_detect's output)
__device__ __forceinline__ void lat_stage_tables(const IcpLattice* __restrict__ L, int ntab, float4* s_tab, int4* s_face, int t, int step) {
    for (int i = t; i < ntab; i += step) s_tab[i] = L->tab[i];
    if (t < LAT_MAX_FACES) {
        const int f = t, w = L->w[f], u = L->fast[f], v = 3 - w - u;
        s_face[f] = make_int4(w, u, L->base[f], __float_as_int(L->c[f]));
        s_face[LAT_MAX_FACES + f] = make_int4(L->toff[u], L->toff[v < 0 || v > 2 ? 0 : v], L->n[u], 0);   // tables of its fast and slow axis (unused faces: anything)
    }
}

// call from every thread of the workgroup; ends with a barrier
template <int THREADS>
__device__ __forceinline__ void lat_stage(const IcpLattice* __restrict__ L, LatFaces& F, float4* s_tab, int4* s_face) {
    lat_faces_load(L, F);
    lat_stage_tables(L, L->ntab, s_tab, s_face, threadIdx.x, THREADS);
    __syncthreads();
}

// m ? a : b for a wave-uniform all-ones / all-zeros word m: ONE v_bfi_b32 with the mask as its scalar operand (written as
// (m & a) | (~m & b) the compiler keeps m AND ~m in scalar registers and issues v_and + v_and_or)
__device__ __forceinline__ float lat_pick(unsigned m, float a, float b) {
    float r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(m), "v"(a), "v"(b));
    return r;
}

// one axis: the table entry nearest to q.  f = fl(fl(q - T[i])^2) at the minimum, t = T[i], gap = f(i - 1) - f(i) (+inf at
// i = 0; negative = not known: the exact test decides), i = ig + di with di in {-1, 0, +1} (left as two flags: only the rare tie walk
// needs the index).  Every axis has a table (one that no face varies along has the single entry 0).
// The window's centre ig only has to be within one entry of the nearest one - all three of the window are evaluated exactly -
// so it is taken from ONE fused multiply-add and a conversion that rounds half up (v_cvt_rpi_i32_f32): q * inv - o * inv sits
// within 1e-4 entries of (q - o) * inv at these magnitudes, against the 7/16 of an entry the uniformity check leaves to spare.
__device__ __forceinline__ void lat_axis(const float4* s_tab, int toff, int n, float o_inv_neg, float inv, float q, float& f, int& ig_out, bool& lo_out,
                                         bool& hi_out, float& t, float& gap) {
    int ig;
    {
        const float pos = __builtin_fmaf(q, inv, o_inv_neg);   // (an approximate position: not one of the canonical operations)
        asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(ig) : "v"(pos));   // floor(pos + 0.5), saturating; NaN -> 0
    }
    ig = min(max(ig, 0), n - 1);   // (one v_med3_i32)
    const float4 W = s_tab[toff + ig];
    const float d0 = __fsub_rn(q, W.x), d1 = __fsub_rn(q, W.y), d2 = __fsub_rn(q, W.z);
    const float f0 = __fmul_rn(d0, d0), f1 = __fmul_rn(d1, d1), f2 = __fmul_rn(d2, d2);
    const float g_mid = __fsub_rn(f0, f1), g_hi = __fsub_rn(f1, f2);
    // (f is unimodal along the table, so f1 > f0 and f1 > f2 cannot both hold: at most one of lo / hi)
    const bool lo = f0 < f1;
    const bool hi = f2 < f1;
    f = f1; t = W.y; gap = g_mid;
    // (lo - the window's centre was one entry too high, so the minimum's own lower neighbour lies outside the window - leaves
    // gap = f0 - f1 < 0: like the 0 it used to be set to, that is below every threshold of the tie filter, and the exact walk
    // decides.  It takes the approximate centre to disagree with the exact comparison: queries within ~1e-4 of an entry of a
    // cell midpoint, which mostly tie and walk anyway - too rare to spend an instruction of the common path on.)
    f = lo ? f0 : f; t = lo ? W.x : t;
    f = hi ? f2 : f; t = hi ? W.z : t; gap = hi ? g_hi : gap;
    ig_out = ig; lo_out = lo; hi_out = hi;
}

// d2 of a face point from the three per-axis terms, canonical association (x + y) + z
__device__ __forceinline__ float lat_sum(float ax, float ay, float az) { return __fadd_rn(__fadd_rn(ax, ay), az); }

struct LatHit {
    float d;            // canonical squared distance to the nearest template point
    float nx, ny, nz;   // that point
    int face;           // its face
    int ix, iy, iz;     // table indices (the constant axis' entry is not used)
};

// (3): the exact walk to the lowest original index among the points of the winning face that tie with the minimum.  Rare (a lane
// enters when its gap is within the rounding of the sum: iteration 0, mid-cell queries): one face at a time.  ix / iy / iz = the
// table indices of the per-axis minima; h.d and h.face are set, h.nx / ny / nz hold the neighbour found so far.
__device__ __forceinline__ void lat_tie_walk(const float4* s_tab, const int4* s_face, const LatFaces& F, float qx, float qy, float qz, float fx, float fy, float fz,
                                             float tx, float ty, float tz, int ix, int iy, int iz, bool maybe, LatHit& h) {
    h.ix = ix; h.iy = iy; h.iz = iz;
    for (int f = 0; f < F.nface; ++f) {
        const bool mine = maybe && h.face == f;
        if (!ballot64(mine)) continue;
        const int4 gd = s_face[f];
        const int w = __builtin_amdgcn_readfirstlane(gd.x), u = __builtin_amdgcn_readfirstlane(gd.y), v = 3 - w - u;   // constant, fast, slow axis
        const float cc = __int_as_float(__builtin_amdgcn_readfirstlane(gd.w));
        const int4 ge = s_face[LAT_MAX_FACES + f];
        const int toff_u = __builtin_amdgcn_readfirstlane(ge.x), toff_v = __builtin_amdgcn_readfirstlane(ge.y);
        const float qw = w == 0 ? qx : (w == 1 ? qy : qz), qu = u == 0 ? qx : (u == 1 ? qy : qz), qv = v == 0 ? qx : (v == 1 ? qy : qz);
        const float dc = __fsub_rn(qw, cc);
        const float fc = __fmul_rn(dc, dc);
        float fu = u == 0 ? fx : (u == 1 ? fy : fz), fv = v == 0 ? fx : (v == 1 ? fy : fz);
        float tu = u == 0 ? tx : (u == 1 ? ty : tz), tv = v == 0 ? tx : (v == 1 ? ty : tz);
        int iu = u == 0 ? h.ix : (u == 1 ? h.iy : h.iz), iv = v == 0 ? h.ix : (v == 1 ? h.iy : h.iz);
        // d2 with the terms of axes u, v, w put back on x, y, z
        auto d_of = [&](float a_u, float a_v) {
            const float ax = w == 0 ? fc : (u == 0 ? a_u : a_v), ay = w == 1 ? fc : (u == 1 ? a_u : a_v), az = w == 2 ? fc : (u == 2 ? a_u : a_v);
            return lat_sum(ax, ay, az);
        };
        // slow axis first (its index is the high part of the original index), then the fast axis at that row
        for (;;) {
            const int j = max(iv - 1, 0);
            const float t = s_tab[toff_v + j].y;
            const float dd = __fsub_rn(qv, t);
            const float a = __fmul_rn(dd, dd);
            const bool go = mine && iv > 0 && d_of(fu, a) == h.d;
            iv = go ? j : iv; fv = go ? a : fv; tv = go ? t : tv;
            if (!ballot64(go)) break;
        }
        for (;;) {
            const int i = max(iu - 1, 0);
            const float t = s_tab[toff_u + i].y;
            const float dd = __fsub_rn(qu, t);
            const float a = __fmul_rn(dd, dd);
            const bool go = mine && iu > 0 && d_of(a, fv) == h.d;
            iu = go ? i : iu; fu = go ? a : fu; tu = go ? t : tu;
            if (!ballot64(go)) break;
        }
        const bool ux = mine && u == 0, uy = mine && u == 1, uz = mine && u == 2, vx = mine && v == 0, vy = mine && v == 1, vz = mine && v == 2;
        h.ix = ux ? iu : (vx ? iv : h.ix); h.nx = ux ? tu : (vx ? tv : h.nx);
        h.iy = uy ? iu : (vy ? iv : h.iy); h.ny = uy ? tu : (vy ? tv : h.ny);
        h.iz = uz ? iu : (vz ? iv : h.iz); h.nz = uz ? tu : (vz ? tv : h.nz);
    }
}

// INDEX: the hit's table indices (and face) are wanted for every query, not only where the walk goes (k_lat_nn).  Until this
// was added k_lat_nn had them only where SOME lane of the wave entered the tie walk - lat_index of any other wave saw zeros and
// returned the face's first point; the existing test interleaves tie queries into every wave and never met it.
// TIES = false: d only (getFitnessScore needs no neighbour).  NF = faces evaluated (3 or LAT_MAX_FACES; the launch's templates
// have at most that many - entries beyond a template's own faces never win)
template <bool TIES, int NF, bool INDEX = false>
__device__ __forceinline__ LatHit lat_nearest(const float4* s_tab, const int4* s_face, const LatFaces& F, float qx, float qy, float qz) {
    float fx, fy, fz, tx, ty, tz, gx, gy, gz;
    int cx, cy, cz;
    bool lox, hix, loy, hiy, loz, hiz;
    LatHit h;
    lat_axis(s_tab, F.tox, F.nx, F.ox, F.ivx, qx, fx, cx, lox, hix, tx, gx);
    lat_axis(s_tab, F.toy, F.ny, F.oy, F.ivy, qy, fy, cy, loy, hiy, ty, gy);
    lat_axis(s_tab, F.toz, F.nz, F.oz, F.ivz, qz, fz, cz, loz, hiz, tz, gz);
    h.ix = h.iy = h.iz = 0;
    h.d = __uint_as_float(0x7f800000u); h.face = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const unsigned m0 = F.m0[f], m1 = F.m1[f], m2 = F.m2[f];
        const float dc = __fsub_rn(lat_pick(m0, qx, lat_pick(m1, qy, qz)), F.c[f]);
        const float fc = __fmul_rn(dc, dc);
        const float d = lat_sum(lat_pick(m0, fc, fx), lat_pick(m1, fc, fy), lat_pick(m2, fc, fz));
        const bool better = d < h.d;   // strict: the first face that reaches the minimum keeps it (4); NaN (no such face): never
        h.d = better ? d : h.d;
        if (TIES) h.face = better ? f : h.face;
    }
    h.nx = tx; h.ny = ty; h.nz = tz;
    if (TIES) {
        // the winning face's constant coordinate replaces its axis' table value; (3): lanes whose lower neighbour along an
        // in-plane axis may round to the same sum take the exact walk
        const int4 fd = s_face[h.face];
        const float c = __int_as_float(fd.w);
        h.nx = fd.x == 0 ? c : tx; h.ny = fd.x == 1 ? c : ty; h.nz = fd.x == 2 ? c : tz;
        const float gsel = fd.x == 0 ? fminf(gy, gz) : (fd.x == 1 ? fminf(gx, gz) : fminf(gx, gy));
        const bool maybe = gsel <= __fmul_rn(h.d, 4.76837158203125e-07f);   // 2^-21
        if (INDEX || ballot64(maybe)) lat_tie_walk(s_tab, s_face, F, qx, qy, qz, fx, fy, fz, tx, ty, tz, cx + (hix ? 1 : 0) - (lox ? 1 : 0), cy + (hiy ? 1 : 0) - (loy ? 1 : 0),
                                          cz + (hiz ? 1 : 0) - (loz ? 1 : 0), maybe, h);
    }
    return h;
}

// (lane's bit of m) ? a : b for a lane mask held in scalar registers: one v_cndmask_b32 (as C++ - a uniform choice between two
// comparison results, then a select - the compiler turns the masks into 0 / 1 vectors and compares them again: six vector
// instructions per choice)
__device__ __forceinline__ float lat_sel(uint64_t m, float a, float b) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}
// fminf of values the compiler cannot see through (results of lat_sel): v_min_f32 returns the other operand for a quiet NaN, which
// is all fminf adds here - none of these values is a signalling NaN - without the v_max x, x the compiler puts in front.
// ASSUMES the IEEE mode bit of compute kernels (the code object's default, .amdhsa_ieee_mode 1; without it v_min_f32 also returns
// the non-NaN operand): tests/test_gpu_lattice_axes.py has NaN and +-inf queries.
__device__ __forceinline__ float lat_min(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float lat_min_inf(float a) {
    float r;
    asm("v_min_f32 %0, 0x7f800000, %1" : "=v"(r) : "v"(a));
    return r;
}

// lat_nearest for a template with at most ONE FACE PER AXIS (IcpLattice::axes_distinct: the three-face cuboid templates).  The
// same rounded operations as the face loop above, without its selects: the distance to the face of constant x is
// (fcx + fy) + fz with fcx = fl(fl(qx - cx)^2), likewise y and z; a missing face's constant is NaN and so is its distance.
// (4) "the first face that reaches the minimum keeps it" = the lexicographic minimum of (d, face index).  Face indices are
// wave-uniform, so a pair (a, b) is decided by one of two comparisons, chosen by a scalar: b wins when d_b < d_a if a comes
// first in the file, when !(d_a < d_b) if b does (or a is missing) - the second form is also true for NaN, which makes a
// missing face lose to any present one and leaves face 0 the winner of a query nothing compares for, as in the face loop.
// The choices are lane masks combined in scalar registers; the neighbour and the tie filter take them as v_cndmask
// conditions - no LDS read of a face descriptor, no branch.  The walk needs the winner as a face number: made inside its branch.
constexpr unsigned LAT_NO_FACE = 99u;   // file position of a face that is not there: after every real one (LAT_MAX_FACES of them at the most)
static_assert(LAT_NO_FACE >= (unsigned)LAT_MAX_FACES && WAVE == 64, "lat_nearest_axes: face order and 64-bit lane masks");
// FACE: h.face is wanted for every query (k_icp_plane: the face's normal), not only where the walk goes.
template <bool TIES, bool INDEX = false, bool FACE = false>
__device__ __forceinline__ LatHit lat_nearest_axes(const float4* s_tab, const int4* s_face, const LatFaces& F, float qx, float qy, float qz) {
    float fx, fy, fz, tx, ty, tz, gx, gy, gz;
    int cx, cy, cz;
    bool lox, hix, loy, hiy, loz, hiz;
    LatHit h;
    lat_axis(s_tab, F.tox, F.nx, F.ox, F.ivx, qx, fx, cx, lox, hix, tx, gx);
    lat_axis(s_tab, F.toy, F.ny, F.oy, F.ivy, qy, fy, cy, loy, hiy, ty, gy);
    lat_axis(s_tab, F.toz, F.nz, F.oz, F.ivz, qz, fz, cz, loz, hiz, tz, gz);
    h.ix = h.iy = h.iz = 0; h.face = 0;
    const float dcx = __fsub_rn(qx, F.cax), dcy = __fsub_rn(qy, F.cay), dcz = __fsub_rn(qz, F.caz);
    const float dx = lat_sum(__fmul_rn(dcx, dcx), fy, fz), dy = lat_sum(fx, __fmul_rn(dcy, dcy), fz), dz = lat_sum(fx, fy, __fmul_rn(dcz, dcz));
    const float inf = __uint_as_float(0x7f800000u);
    if (!TIES) {
        h.d = fminf(fminf(fminf(dx, dy), dz), inf);   // (NaN-ignoring: the least distance of the faces there are, +inf when nothing compares)
        h.nx = tx; h.ny = ty; h.nz = tz;
        return h;
    }
    // file order of the faces, a missing one last (uniform); the lane masks of the four comparisons, combined in scalar registers
    const unsigned ox = F.afx < 0 ? LAT_NO_FACE : (unsigned)F.afx, oy = F.afy < 0 ? LAT_NO_FACE : (unsigned)F.afy, oz = F.afz < 0 ? LAT_NO_FACE : (unsigned)F.afz;
    const uint64_t wy = oy < ox ? ballot64(!(dx < dy)) : ballot64(dy < dx);   // y beats x
    const float dxy = lat_sel(wy, dy, dx);
    const uint64_t z_first = (oz < oy ? wy : 0ull) | (oz < ox ? ~wy : 0ull);   // z comes before the better of x and y
    const uint64_t wz = ballot64(dz < dxy) | (z_first & ballot64(!(dxy < dz)));   // z beats it
    h.d = lat_min_inf(lat_sel(wz, dz, dxy));                                    // (NaN - a query with a NaN coordinate - becomes the loop's +inf)
    const uint64_t win_x = ~(wy | wz);
    h.nx = lat_sel(win_x, F.cax, tx); h.ny = lat_sel(wy & ~wz, F.cay, ty); h.nz = lat_sel(wz, F.caz, tz);
    // (3): the lesser gap of the winning face's two in-plane axes - x wins: min(gy, gz), y: min(gx, gz), z: min(gx, gy)
    const float gsel = lat_min(lat_sel(win_x, gy, gx), lat_sel(wz, gy, gz));
    const bool maybe = gsel <= __fmul_rn(h.d, 4.76837158203125e-07f);   // 2^-21
    if (FACE) {
        const int lane = (int)(threadIdx.x & (WAVE - 1));
        h.face = (wz >> lane) & 1 ? F.afz : ((wy >> lane) & 1 ? F.afy : F.afx);
    }
    if (INDEX || ballot64(maybe)) {
        const int lane = (int)(threadIdx.x & (WAVE - 1));   // (bit of this lane in a mask: 64-wide waves, one-dimensional blocks - every kernel here)
        h.face = (wz >> lane) & 1 ? F.afz : ((wy >> lane) & 1 ? F.afy : F.afx);
        lat_tie_walk(s_tab, s_face, F, qx, qy, qz, fx, fy, fz, tx, ty, tz, cx + (hix ? 1 : 0) - (lox ? 1 : 0), cy + (hiy ? 1 : 0) - (loy ? 1 : 0),
                     cz + (hiz ? 1 : 0) - (loz ? 1 : 0), maybe, h);
    }
    return h;
}

// the search of a query against whatever template F describes (uniform choices): one face per axis, at most three faces, any
template <bool TIES, bool FACE = false>
__device__ __forceinline__ LatHit lat_nearest_any(const float4* s_tab, const int4* s_face, const LatFaces& F, float qx, float qy, float qz) {
    return F.axes ? lat_nearest_axes<TIES, false, FACE>(s_tab, s_face, F, qx, qy, qz)
                  : (F.nface <= 3 ? lat_nearest<TIES, 3>(s_tab, s_face, F, qx, qy, qz) : lat_nearest<TIES, LAT_MAX_FACES>(s_tab, s_face, F, qx, qy, qz));
}

// original index of a hit (the diagnostic entry point; the ICP itself only needs the neighbour's coordinates)
__device__ __forceinline__ int lat_index(const int4* s_face, const LatFaces& F, const LatHit& h) {
    const int4 fd = s_face[h.face];
    const int w = fd.x, u = fd.y, v = 3 - w - u;
    const int iu = u == 0 ? h.ix : (u == 1 ? h.iy : h.iz), iv = v == 0 ? h.ix : (v == 1 ? h.iy : h.iz);
    return fd.z + iv * s_face[LAT_MAX_FACES + h.face].z + iu;
}

// Rule C4's fixed-point term rint(v * 2^SHIFT) WITHOUT taking it out of the double: u = (double)v + 1.5 * 2^(52 - SHIFT) is ONE
// rounded addition (v is exact as a double; nearest even at 2^-SHIFT, the spacing of doubles in [2^(52-SHIFT), 2^(53-SHIFT))),
// and for |v * 2^SHIFT| < 2^50 the BITS of u, read as an integer, are C + rint(v * 2^SHIFT) with C = the bits of the constant.
// So a lane adds the raw bits to its 64-bit accumulator - cvt, one v_add_f64 with the constant as a scalar operand, one 64-bit
// add - and since every POINT adds exactly one term to each sum, the solver takes n x C off each sum again (mod 2^64, like the
// sums themselves).  (Until the end of round 5 this was fma(v, 2^SHIFT, 1.5 * 2^52): the same integers, but the compiler
// rebuilt the addend in a register pair before every fma - two moves per term.)
template <int SHIFT>
struct LatFix {
    static constexpr unsigned long long C = ((unsigned long long)(1023 + 52 - SHIFT) << 52) | (1ull << 51);   // bits of 1.5 * 2^(52 - SHIFT)
    static __device__ __forceinline__ unsigned long long bits(float v) {
        return (unsigned long long)__double_as_longlong(__dadd_rn((double)v, __longlong_as_double((long long)C)));
    }
    // the same integer for ANY v, by the general conversion
    static __device__ __forceinline__ unsigned long long general(float v) { return (unsigned long long)fixq(v, SHIFT) + C; }
};
// N terms -> the N integers a point adds to its sums: term D2 at FIX_SHIFT_D2, the others at FIX_SHIFT.  raw: the caller's range
// test says that every term is inside LatFix's range (a per-rule fact); the same integers either way.
template <int D2, int N>
__device__ __forceinline__ void lat_fix_terms(const float (&t)[N], bool raw, unsigned long long (&b)[N]) {
    static_assert(D2 >= 0 && D2 < N, "the squared-distance term is one of the N");
    if (raw) {
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = i == D2 ? LatFix<FIX_SHIFT_D2>::bits(t[i]) : LatFix<FIX_SHIFT>::bits(t[i]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = i == D2 ? LatFix<FIX_SHIFT_D2>::general(t[i]) : LatFix<FIX_SHIFT>::general(t[i]);
    }
}
// the one term of a fitness sum (a squared distance; raw bits below (128 m)^2)
__device__ __forceinline__ unsigned long long lat_fix_d2(float d) { return d < 16384.f ? LatFix<FIX_SHIFT_D2>::bits(d) : LatFix<FIX_SHIFT_D2>::general(d); }
// what `count` points have added to a sum on top of its terms (is_d2: the sum of the FIX_SHIFT_D2 term): the solver takes it off
__device__ __forceinline__ unsigned long long lat_fix_offset(bool is_d2, unsigned long long count) {
    return count * (is_d2 ? LatFix<FIX_SHIFT_D2>::C : LatFix<FIX_SHIFT>::C);
}
static_assert(LatFix<32>::C == 0x4138000000000000ull && LatFix<36>::C == 0x40f8000000000000ull, "constants of lat_fix");
static_assert(FIX_SHIFT == 32 && FIX_SHIFT_D2 == 36, "k_icp_lat's moment sums are written for these scales");

// The passes of wave `sub` of WAVES over the n >= 1 points at pts, 64 at a time: body(myq, act, p) with myq = the lane's point,
// act = it exists, p = its record (the last point's where it does not).  The points of the next pass are requested before the
// current pass is worked on: one wave per SIMD per cluster has nothing else to cover an L2 round trip with.  body may store to
// pts[myq]: a later pass never reads it.
template <int WAVES, class Body>
__device__ __forceinline__ void lat_for_passes(const float4* pts, int n, int sub, int lane, Body body) {
    const int npass = (n + 63) >> 6;
    float4 pnext = pts[min((sub << 6) + lane, n - 1)];
    for (int pss = sub; pss < npass; pss += WAVES) {
        const int myq = (pss << 6) + lane;
        const bool act = myq < n;
        const float4 p = pnext;
        pnext = pts[min(((pss + WAVES) << 6) + lane, n - 1)];
        body(myq, act, p);
    }
}

// The last step of an ICP, by wave `sub` of WAVES: X <- T X in place (PCL transforms before it tests convergence), then
// getFitnessScore() of Tfinal * original source - every point's d2 as one rule-C4 sum (n x LatFix<FIX_SHIFT_D2>::C on top),
// folded into acc[0] (LDS).  so: the cluster's state in LDS, read as uniform values; both arrays are prefetched.
template <int WAVES>
__device__ __forceinline__ void lat_fitness_pass(float4* pts, const float4* pts0, int n, int sub, int lane, const IcpState& so, const float4* tab,
                                                 const int4* face, const LatFaces& F, unsigned long long* acc) {
    const int npass = (n + 63) >> 6;
    float T[12], Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        T[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(so.T[i])));
        Tf[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(so.Tfinal[i])));
    }
    unsigned long long S[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0ull;
    float4 pnext = pts[min((sub << 6) + lane, n - 1)], p0next = pts0[min((sub << 6) + lane, n - 1)];
    for (int pss = sub; pss < npass; pss += WAVES) {
        const int myq = (pss << 6) + lane;
        const bool act = myq < n;
        const float4 p = pnext, p0 = p0next;
        pnext = pts[min(((pss + WAVES) << 6) + lane, n - 1)];
        p0next = pts0[min(((pss + WAVES) << 6) + lane, n - 1)];
        float ox, oy, oz;
        xform(T, p.x, p.y, p.z, ox, oy, oz);
        if (act) pts[myq] = make_float4(ox, oy, oz, p.w);
        float qx, qy, qz;
        xform(Tf, p0.x, p0.y, p0.z, qx, qy, qz);
        const LatHit h = lat_nearest_any<false>(tab, face, F, qx, qy, qz);
        if (act) S[0] += lat_fix_d2(h.d);
    }
    if (sub < npass) wave_fold_to_lds(S, 1, acc);
}

}  // namespace cd
