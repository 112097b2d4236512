// icp_search.hpp - device-only: the exact nearest-neighbour primitives shared by k_icp.hip, k_icp_cluster.hip and k_icp_pipe.hip.
#pragma once
#include "kernels.hpp"

// trips and active lanes of grid_search's two loops: k_icp_pipe.hip, which owns the counters, defines it in -DCD_STATS builds
#ifndef CD_GRID_STAT
#define CD_GRID_STAT(slot, cond)
#endif

namespace cd {

// ---------------------------------------------------------------------------------------
// Exact nearest-neighbour search, "transposed": a wave owns ONE query at a time and its 64
// lanes scan 64 template points per step out of LDS (one conflict-free ds_read_b128 per lane).
//
// The template is cut into runs of 64 consecutive points, each with an axis-aligned box
// [lo,hi] (built at cd_set_template).  For a query q the bound
//   e_a = max(lo_a - q_a, q_a - hi_a, 0),  lb = (e_x*e_x + e_y*e_y) + e_z*e_z
// evaluated with the canonical association satisfies lb <= d2(q,p) for EVERY p in the run in
// float arithmetic, because each step (rounded subtraction, square, rounded sum) is monotone
// in |component|.  Lane l keeps the boxes of runs l and l+64 of the staged chunk in registers,
// so ONE ballot per 64 runs yields the wave-uniform set of runs that can still hold a point
// with d2 <= best; every other run is skipped without touching it.  This is pruning, not
// approximation: no candidate that could improve on or tie the current best is dropped.
// Seeding: best enters as nextafter(d2(q, seed)) with the previous iteration's neighbour as
// seed; an ascending strict-< scan from that state still ends at the lowest index achieving
// the global minimum (rule C5) - each lane keeps the first minimum of its own ascending
// subsequence and the wave reduction takes the lexicographic minimum of (d2 bits, index).
// ---------------------------------------------------------------------------------------
constexpr int ICPT_THREADS = 1024;                 // 16 waves, 4 per SIMD
constexpr int ICPT_WAVES = ICPT_THREADS / WAVE;
constexpr int ICPT_TPL_LDS = ICP_TPL_LDS;          // template points resident in LDS per pass (119 runs, 119 KiB)
constexpr int ICPT_IMG = ICPT_TPL_LDS + ICP_SUB;   // + one pad run

__device__ __forceinline__ float next_up_nonneg(float d) { return __uint_as_float(__float_as_uint(d) + 1u); }
__device__ __forceinline__ float seed_bound(float d0) { return d0 < 3.0e38f ? next_up_nonneg(d0) : __uint_as_float(0x7f800000u); }

// (e_a = max(lo_a - q_a, q_a - hi_a, 0) is |q_a - clamp(q_a, lo_a, hi_a)|: one v_med3_f32 and one subtraction per axis instead of
// two subtractions and a v_max3 - the squares are the same floats, the sign is gone after squaring.  An inverted (empty) box
// gives 0 instead of "never": it is not pruned, which costs a test and no correctness.)
__device__ __forceinline__ float box_lb(const float4& L, const float4& H, float x, float y, float z) {
    const float ex = __fsub_rn(x, __builtin_amdgcn_fmed3f(x, L.x, H.x));
    const float ey = __fsub_rn(y, __builtin_amdgcn_fmed3f(y, L.y, H.y));
    const float ez = __fsub_rn(z, __builtin_amdgcn_fmed3f(z, L.z, H.z));
    return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}

// min over the 64 lanes of a non-negative float, by DPP row shifts + row broadcasts (no LDS).
// Non-negative floats order like their bit patterns, so the reduction is an unsigned integer min.
__device__ __forceinline__ float wave_min_f32_nonneg(float v) {
    unsigned x = __float_as_uint(v);
#define CD_DPP_MIN(ctrl, rowmask) x = min(x, (unsigned)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)x, ctrl, rowmask, 0xf, false));
    CD_DPP_MIN(0x111, 0xf)   // row_shr:1
    CD_DPP_MIN(0x112, 0xf)   // row_shr:2
    CD_DPP_MIN(0x114, 0xf)   // row_shr:4
    CD_DPP_MIN(0x118, 0xf)   // row_shr:8   -> lane 15 of every row holds the row minimum
    CD_DPP_MIN(0x142, 0xa)   // row_bcast:15 into rows 1,3
    CD_DPP_MIN(0x143, 0xc)   // row_bcast:31 into rows 2,3 -> lane 63 holds the wave minimum
#undef CD_DPP_MIN
    return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)x, 63));
}

// Boxes of runs `lane` and `lane+64` of the staged chunk, kept in registers.
struct RunBoxes { float4 L0, H0, L1, H1; };

// Stage template chunk [c0, c0+cn) into LDS: the chunk, its last run padded to 64 points, plus one
// whole pad run; pad points sit at +inf with original index INT_MAX, so their distance is +inf and
// they can never win (removes every bounds predicate from the search).  Ends with a barrier.
__device__ __forceinline__ void stage_chunk(const float4* __restrict__ tpl, const float4* __restrict__ blo,
                                            const float4* __restrict__ bhi, int c0, int cn, float4* s_tpl, RunBoxes& bx) {
    const int lane = threadIdx.x & 63;
    const int nruns = (cn + ICP_SUB - 1) / ICP_SUB;
    const float inf = __uint_as_float(0x7f800000u);
    __syncthreads();
    for (int k = threadIdx.x; k < (nruns + 1) * ICP_SUB; k += ICPT_THREADS)
        s_tpl[k] = k < cn ? tpl[c0 + k] : make_float4(inf, inf, inf, __int_as_float(0x7fffffff));
    bx.L0 = make_float4(inf, inf, inf, 0.f); bx.H0 = bx.L0; bx.L1 = bx.L0; bx.H1 = bx.L0;
    if (lane < nruns) { bx.L0 = blo[c0 / ICP_SUB + lane]; bx.H0 = bhi[c0 / ICP_SUB + lane]; }
    if (lane + 64 < nruns) { bx.L1 = blo[c0 / ICP_SUB + lane + 64]; bx.H1 = bhi[c0 / ICP_SUB + lane + 64]; }
    __syncthreads();
}

// Per-wave query state: lane k of a wave holds query (wave + 16*k) of the slice.
struct QueryRegs { float px, py, pz, pbest; int pbi, poi; };

// The seed of a lane's query (q.px, q.py, q.pz set): the previous neighbour (use_prev; *prev is read only then) and/or,
// `coarse`, the first point of every 64-point run, the lowest index winning ties.  Leaves the seed bound in q.pbest, the
// seed's position in q.pbi and its original index in q.poi.  (k_icp_pipe.hip seeds the same way from its own image: seed_at.)
__device__ __forceinline__ void seed_query(const float4* __restrict__ tpl, int m, bool use_prev, bool coarse, const int* prev, QueryRegs& q) {
    q.pbest = 3.402823466e38f;
    if (use_prev) {
        q.pbi = *prev;
        const float4 q0 = tpl[q.pbi];
        q.pbest = dist2(q.px, q.py, q.pz, q0.x, q0.y, q0.z);
    }
    if (coarse) {
        for (int j = 0; j < m; j += ICP_SUB) {
            const float4 t = tpl[j];
            const float d = dist2(q.px, q.py, q.pz, t.x, t.y, t.z);
            if (d < q.pbest) { q.pbest = d; q.pbi = j; }
        }
    }
    q.pbest = seed_bound(q.pbest);
    q.poi = __float_as_int(tpl[q.pbi].w);
}

__device__ __forceinline__ unsigned long long lanes_below(int nk) { return nk >= 64 ? ~0ull : ((1ull << nk) - 1ull); }

// ---------------------------------------------------------------------------------------
// Exact nearest-neighbour search, lane-per-query over the template's uniform grid.
//
// Once ICP has pulled the cloud onto the template, a query's seed (its neighbour of the previous
// iteration) is millimetres away, and the ball of that radius touches a handful of grid cells.
// The template is stored sorted by cell (IcpGrid, common.hpp), so the cells cx0..cx1 of one
// (cy,cz) row are one contiguous range of stored points: a lane walks the rows of its ball's
// cell box and tests every point in them with the canonical dist2 and the lexicographic
// (d2, original index) update.  Exactness: with bound = nextafter(d2(q, seed)) and
//   rr = sqrt(bound)*(1+2e-6),  r_a = rr + 4e-7*|q_a| + 1e-7   (slack > rounding of q_a -+ r_a),
// every template point p outside the cell box has |q_a - p_a| > rr on some axis a (the cell
// coordinate is the same monotone float function on host and device), hence float
// d2(q,p) >= rr^2*(1-5u) > bound: it can neither beat nor tie the seed.  Every point inside the
// box is tested.  So the result equals the full scan's.  Queries whose ball is wider than
// IcpParams::grid_rc cells (early iterations) are left to the wave-per-query searches.
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ int grid_coord(float v, float o, float inv, int n) {
    const float t = floorf(__fmul_rn(__fsub_rn(v, o), inv));
    return t >= (float)(n - 1) ? n - 1 : (t > 0.f ? (int)t : 0);
}

// q.pbest holds the seed bound on entry; `act` lanes search, the others idle through the loop.
//
// Row pruning: the cell box is the bounding cube of the ball, but the ball itself only reaches a few of its
// rows.  For a row (cy,cz), e_y / e_z = distance from q to the row's slab on that axis, reduced by a slack
// that covers every float rounding of the cell boundaries (so they are lower bounds of |q_y-p_y|, |q_z-p_z|
// for every point p filed in the row).  A point that can still beat or tie the seed has real
// dx^2 <= bound*(1+5u) - (dy^2+dz^2) <= rem := rr2 - e2*(1-1e-6); rem < 0 skips the row, otherwise the x-range
// shrinks to the cells of q_x -+ sqrt(rem).
// The point loop has no divergent branch: a lane without a point to test reads the +inf pad point `pad`, whose key can never
// win.  (A select-only version of the row step was measured too: same time, so the row step keeps its early-outs.)
// SH = bits of the stored position in the low word of a key: 13 for an LDS-resident template (positions and original
// indices < 2^13, "no index" = 0x7fffffff), 16 for a template read from global memory (both < 2^16, "no index" = all ones).
template <int SH>
struct KeyFmt {
    static constexpr unsigned NONE = SH == 13 ? 0x7fffffffu : 0xffffffffu;
    static constexpr unsigned POS_MASK = (1u << SH) - 1u;
};
// PK: the template image's .w already holds the key's low word (original index << SH | stored position): k_icp_pipe re-labels
// its LDS image that way once, which takes one vector instruction per tested point out of both searches
template <int SH = 13, bool PK = false, bool SK = false>
__device__ __forceinline__ void grid_search(const float4* s_tpl, const unsigned short* s_cs, const IcpGrid& g, bool act, float rr,
                                            QueryRegs& q, int pad) {
    // running minimum as (d2 bits : original index): the lexicographic update of rule C5 is then ONE unsigned 64-bit compare
    // (no branch, no tie special case; the seed bound enters with "no index" = INT_MAX, so the seed point itself beats it).
    // SK (k_icp_pipe / k_icp_pipe_big since round 4): the caller hands over the SEED'S OWN KEY - q.pbest = d2(q, seed) exactly,
    // q.poi = the seed's key word ("no index" when there is no seed) - so the minimum starts at the seed and only a strictly
    // better candidate (closer, or as close with a lower original index) moves it: same result, and a query whose neighbour
    // did not change needs no write-back
    unsigned long long lkey = ((unsigned long long)__float_as_uint(q.pbest) << 32) | (unsigned long long)(SK ? (unsigned)q.poi : KeyFmt<SH>::NONE);
    const float slx = __fadd_rn(__fmul_rn(4.0e-7f, __fadd_rn(__fadd_rn(fabsf(q.px), fabsf(g.ox)), __fmul_rn((float)g.nx, g.cell))), 1.0e-7f);
    const float sly = __fadd_rn(__fmul_rn(4.0e-7f, __fadd_rn(__fadd_rn(fabsf(q.py), fabsf(g.oy)), __fmul_rn((float)g.ny, g.cell))), 1.0e-7f);
    const float slz = __fadd_rn(__fmul_rn(4.0e-7f, __fadd_rn(__fadd_rn(fabsf(q.pz), fabsf(g.oz)), __fmul_rn((float)g.nz, g.cell))), 1.0e-7f);
    const float ryy = __fadd_rn(rr, sly), rzz = __fadd_rn(rr, slz);
    const int y0 = grid_coord(__fsub_rn(q.py, ryy), g.oy, g.inv, g.ny), y1 = grid_coord(__fadd_rn(q.py, ryy), g.oy, g.inv, g.ny);
    const int z1 = grid_coord(__fadd_rn(q.pz, rzz), g.oz, g.inv, g.nz);
    int ry = y0, rz = grid_coord(__fsub_rn(q.pz, rzz), g.oz, g.inv, g.nz);
    const float rr2 = __fmul_rn(__fmul_rn(rr, rr), 1.0f + 1.0e-6f);
    const float huge = 3.0e38f;
    // Row advance WITHOUT divergent control flow (round 4): written with nested ifs (if (need) { if (rz > z1) .. else { .. if (rem
    // >= 0) .. } }, rounds 1-3) it compiled to ~35 scalar instructions per trip - exec-mask saves and restores, the live booleans
    // as scalar masks - on a scalar unit that sixteen waves share: 4.31 -> 4.19 ms for the kernel (profiles/r04_salu_diet_ab.txt).
    // Here "needs a row" is (i >= b && rz <= z1) - a lane whose walk is over, or that takes no part, has rz beyond z1 and
    // b = INT_MIN - every lane computes the row's range, and selects decide who takes it: one ballot per trip.
    int i = 0, b = act ? 0 : (-0x7fffffff - 1);
    if (!act) rz = z1 + 1;
    bool more = act;   // (only read by the loop exit below)
    for (;;) {
        for (;;) {
            const bool adv = i >= b && rz <= z1;
            if (!ballot64(adv)) break;
            CD_GRID_STAT(4, adv)
            const int cz = min(rz, g.nz - 1);   // (address arithmetic of lanes that are done stays inside the table)
            const float ylo = ry == 0 ? -huge : __fadd_rn(g.oy, __fmul_rn((float)ry, g.cell));
            const float yhi = ry == g.ny - 1 ? huge : __fadd_rn(g.oy, __fmul_rn((float)(ry + 1), g.cell));
            const float zlo = cz == 0 ? -huge : __fadd_rn(g.oz, __fmul_rn((float)cz, g.cell));
            const float zhi = cz == g.nz - 1 ? huge : __fadd_rn(g.oz, __fmul_rn((float)(cz + 1), g.cell));
            const float ey = fmaxf(__fsub_rn(fmaxf(__fsub_rn(ylo, q.py), __fsub_rn(q.py, yhi)), sly), 0.f);
            const float ez = fmaxf(__fsub_rn(fmaxf(__fsub_rn(zlo, q.pz), __fsub_rn(q.pz, zhi)), slz), 0.f);
            const float e2 = __fmul_rn(__fadd_rn(__fmul_rn(ey, ey), __fmul_rn(ez, ez)), 1.0f - 1.0e-6f);
            const float rem = __fsub_rn(rr2, e2);
            const bool hit = adv && rem >= 0.f;
            const float rx = __fadd_rn(__fmul_rn(__builtin_amdgcn_sqrtf(fmaxf(rem, 0.f)), 1.0f + 1.0e-6f), slx);
            const int row = (cz * g.ny + ry) * g.nx;
            const int ni = s_cs[row + grid_coord(__fsub_rn(q.px, rx), g.ox, g.inv, g.nx)];
            const int nb = s_cs[row + grid_coord(__fadd_rn(q.px, rx), g.ox, g.inv, g.nx) + 1];
            i = hit ? ni : i;
            b = hit ? nb : b;
            const bool wrap = ry >= y1;
            rz = (adv && wrap) ? rz + 1 : rz;
            ry = adv ? (wrap ? y0 : ry + 1) : ry;
        }
        more = i < b;
        if (!ballot64(more)) break;
        // B: test the points of the current ranges, two per trip.  No lane is switched off: a lane whose range is used up (or
        // whose walk is over) simply tests the points that follow it - real template points, which can never displace the true
        // neighbour - clamped to the +inf pad point.  The low word of the key is (original index << 13 | stored position), so
        // the winner's position needs no select of its own.
        while (ballot64(i < b)) {
            CD_GRID_STAT(6, i < b)
            if constexpr (SH == 16) {
                // template in global memory: a trip costs an L2 round trip, so four points are in flight per trip
                const int i0 = min(i, pad), i1 = min(i + 1, pad), i2 = min(i + 2, pad), i3 = min(i + 3, pad);
                const float4 t = s_tpl[(unsigned)i0];
                const float4 u = s_tpl[(unsigned)i1];
                const float4 v = s_tpl[(unsigned)i2];
                const float4 w = s_tpl[(unsigned)i3];
                const float d = dist2(q.px, q.py, q.pz, t.x, t.y, t.z);
                const float e = dist2(q.px, q.py, q.pz, u.x, u.y, u.z);
                const float f = dist2(q.px, q.py, q.pz, v.x, v.y, v.z);
                const float h = dist2(q.px, q.py, q.pz, w.x, w.y, w.z);
                const unsigned long long kd_ = ((unsigned long long)__float_as_uint(d) << 32) | (((unsigned)__float_as_int(t.w) << SH) | (unsigned)i0);
                const unsigned long long ke_ = ((unsigned long long)__float_as_uint(e) << 32) | (((unsigned)__float_as_int(u.w) << SH) | (unsigned)i1);
                const unsigned long long kf_ = ((unsigned long long)__float_as_uint(f) << 32) | (((unsigned)__float_as_int(v.w) << SH) | (unsigned)i2);
                const unsigned long long kh_ = ((unsigned long long)__float_as_uint(h) << 32) | (((unsigned)__float_as_int(w.w) << SH) | (unsigned)i3);
                lkey = kd_ < lkey ? kd_ : lkey;
                lkey = ke_ < lkey ? ke_ : lkey;
                lkey = kf_ < lkey ? kf_ : lkey;
                lkey = kh_ < lkey ? kh_ : lkey;
                i += 4;
            } else {
            // two points per trip, (i, i + 1), clamped together: one address, the second point 16 bytes on
            const int i0 = min(i, pad - 1), i1 = i0 + 1;
            const float4 t = s_tpl[(unsigned)i0];
            const float4 u = s_tpl[(unsigned)i1];
            // (PK images are stored (x, y, key word, z))
            const float d = dist2(q.px, q.py, q.pz, t.x, t.y, PK ? t.w : t.z);
            const float e = dist2(q.px, q.py, q.pz, u.x, u.y, PK ? u.w : u.z);
            unsigned long long kd_ = ((unsigned long long)__float_as_uint(d) << 32) | (PK ? (unsigned)__float_as_int(t.z) : (((unsigned)__float_as_int(t.w) << SH) | (unsigned)i0));
            unsigned long long ke_ = ((unsigned long long)__float_as_uint(e) << 32) | (PK ? (unsigned)__float_as_int(u.z) : (((unsigned)__float_as_int(u.w) << SH) | (unsigned)i1));
            // (opaque to the optimiser: compare AND select then use the key's own register pair, so the distance is formed in
            // its high half instead of being copied there)
            asm("" : "+v"(kd_));
            asm("" : "+v"(ke_));
            lkey = kd_ < lkey ? kd_ : lkey;
            lkey = ke_ < lkey ? ke_ : lkey;
            i += 2;
            }
        }
    }
    const unsigned lo = (unsigned)(lkey & 0xffffffffull);
    if (act && lo != KeyFmt<SH>::NONE) { q.pbest = __uint_as_float((unsigned)(lkey >> 32)); q.pbi = (int)(lo & KeyFmt<SH>::POS_MASK); q.poi = SK ? (int)lo : (int)(lo >> SH); }
}

// Search the staged chunk for the queries of this wave whose bit is set in `todo` (wave-uniform); updates q in place.
__device__ __forceinline__ void search_chunk(const float4* s_tpl, const RunBoxes& bx, int c0, int cn, QueryRegs& q,
                                             unsigned long long todo) {
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int k = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.px), k));
        const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.py), k));
        const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.pz), k));
        const float best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.pbest), k));
        // Lanes start from (bound, no index): a lane can only be selected below if it beat `best`, and the
        // seed point itself always does in the chunk that holds it.  Only when `best` is a real distance
        // carried over from a lower chunk (c0 > 0) must ties against the carried neighbour be decided,
        // so only then is its original index needed.
        const int boi = c0 > 0 ? __builtin_amdgcn_readlane(q.poi, k) : 0x7fffffff;
        unsigned long long m0 = ballot64(box_lb(bx.L0, bx.H0, x, y, z) <= best);
        unsigned long long m1 = ballot64(box_lb(bx.L1, bx.H1, x, y, z) <= best);
        float lbest = best;
        int lbi = 0, loi = boi;
        // Visit the surviving runs (1.5 per query on average, so no unrolling/padding).  The template is stored
        // re-tiled into compact 64-point patches, so candidates are NOT met in original-index
        // order: the update is the lexicographic (d2, original index) comparison (rule C5).
#define CD_TAKE(dd, tt, rr)                                                                     \
        {                                                                                       \
            const int oi_ = __float_as_int(tt.w);                                               \
            const bool up_ = (dd < lbest) || (dd == lbest && oi_ < loi);                        \
            lbest = up_ ? dd : lbest; lbi = up_ ? c0 + rr * ICP_SUB + lane : lbi; loi = up_ ? oi_ : loi; \
        }
#define CD_VISIT2(mask, base)                                                                   \
        while (mask) {                                                                          \
            const int r0 = (base) + __ffsll((long long)mask) - 1; mask &= mask - 1;             \
            const float4 t0 = s_tpl[r0 * ICP_SUB + lane];                                       \
            const float d0 = dist2(x, y, z, t0.x, t0.y, t0.z);                                  \
            CD_TAKE(d0, t0, r0)                                                                 \
        }
        CD_VISIT2(m0, 0)
        CD_VISIT2(m1, 64)
#undef CD_VISIT2
#undef CD_TAKE
        // lexicographic (d2, original index) minimum over the wave.  Only lanes that beat the incoming
        // bound can hold it; when exactly one did (the usual case once seeds are tight) it IS the answer
        // and three v_readlane replace the reduction.  Otherwise: min distance by DPP, then the lowest
        // original index among the lanes that hold it.
        const unsigned long long imp = ballot64(lbest < best || (lbest == best && loi < boi));
        if (imp == 0) continue;   // nothing in this chunk beats the carried neighbour (multi-chunk templates only)
        float dmin;
        int rbi, roi;
        if (__popcll(imp) == 1) {
            const int l = __ffsll((long long)imp) - 1;
            dmin = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lbest), l));
            rbi = __builtin_amdgcn_readlane(lbi, l);
            roi = __builtin_amdgcn_readlane(loi, l);
        } else {
            dmin = wave_min_f32_nonneg(lbest);
            unsigned long long eq = ballot64(lbest == dmin);
            rbi = 0; roi = 0x7fffffff;
            while (eq) {
                const int l = __ffsll((long long)eq) - 1;
                eq &= eq - 1;
                const int oi_ = __builtin_amdgcn_readlane(loi, l);
                const int bi_ = __builtin_amdgcn_readlane(lbi, l);
                if (oi_ <= roi) { roi = oi_; rbi = bi_; }
            }
        }
        if (lane == k) { q.pbest = dmin; q.pbi = rbi; q.poi = roi; }
    }
}

// One template of the arena: its points and the boxes of its 64-point runs.
struct TplRef { const float4 *p, *lo, *hi; };
__device__ __forceinline__ TplRef tpl_ref(const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                          const float4* __restrict__ thi, int off) {
    return {tpl + off, tlo + off / ICP_SUB, thi + off / ICP_SUB};
}

// A template without a chunk table that does not fit LDS: every query against every ICPT_TPL_LDS points of it in turn.
// The image left in LDS is a part of the template: the caller's `staged` must become -1.
__device__ __forceinline__ void search_fixed_chunks(const TplRef& t, int m, QueryRegs& q, int nk, float4* s_tpl, RunBoxes& bx) {
    for (int c0 = 0; c0 < m; c0 += ICPT_TPL_LDS) {
        const int cn = min(ICPT_TPL_LDS, m - c0);
        stage_chunk(t.p, t.lo, t.hi, c0, cn, s_tpl, bx);
        search_chunk(s_tpl, bx, c0, cn, q, lanes_below(nk));
    }
}

}  // namespace cd
