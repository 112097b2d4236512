// k_prism.hip - canonical rule C20: the table prism (prism_math.hpp holds the arithmetic, perception_amd/table_prism.py the
// specification).
//
// One kernel on the context's stream, one workgroup per row (a frame of a fused call, or the one cloud of cd_table_prism):
//   A. extremes   every plane inlier is quantised (steps 1 - 5) and the workgroup reduces eight 64-bit integer keys - the
//                 inliers' extreme points to the left, lower left, bottom ... upper left, each (direction value, tie-breaker),
//                 so the eight points do not depend on the order of the visits.  The left one is the lexicographically smallest
//                 point: the hull's first vertex.
//   B. prune      the inliers are quantised again (fifteen double operations against a second array of the context's size)
//                 and those strictly inside the polygon of the eight are dropped: they are strictly inside the hull.  The
//                 survivors go to the row's scratch in global memory and, the first PRISM_LDS_POINTS of them, to LDS, in
//                 whatever order the waves arrive: the hull is a set.
//   C. march      from the first vertex, one workgroup-wide reduction per hull vertex over the survivors (LDS when they all
//                 fit, global memory otherwise): the most clockwise point as seen from the current vertex, ties to the farthest
//                 - an exact int64 comparator, and a strict weak order because all points lie within less than a half turn as
//                 seen from a hull vertex.  No sort; the march stops at the first vertex, at a row whose points are all one,
//                 or at vertex PRISM_MAX_HULL + 1 (overflow).  Its length is bounded by that cap whatever the data.
//   D. select     the workgroup walks the object cloud tile by tile, classifies every point (step 7; the hull is in LDS, read at
//                 one address by all lanes) and compacts the kept points in order - whole float4 records - as k_outlier_select
//                 does; it writes the map (index in the kept row, or -1), the kept indices, the row's record and new count.
// A row without a plane (have == 0) passes untouched: every point kept, the record zero but for the counts.
//
// Every count read from memory is clamped to the row it indexes before it bounds a loop, every plane index is clamped into the
// row it reads, a survivor's slot is below the number of inliers and a kept point's place not above its own index.
#include <climits>

#include "kernels.hpp"
#include "outlier_math.hpp"
#include "prism_math.hpp"

namespace cd {

constexpr long long PRISM_NO_KEY = LLONG_MIN;

static_assert(sizeof(PrismPoint) == sizeof(int2), "a survivor is one int2 of the scratch row");

__device__ __forceinline__ long long prism_key(int32_t w, int32_t t) { return (long long)w * 4294967296ll + ((long long)t + 2147483648ll); }
__device__ __forceinline__ int32_t prism_key_w(long long k) { return (int32_t)(k >> 32); }
__device__ __forceinline__ int32_t prism_key_t(long long k) { return (int32_t)((long long)(k & 0xffffffffll) - 2147483648ll); }

// R inliers of a lane, first + j * BLOCK: every index is loaded, then every point, before any is used - an inlier is two dependent
// round trips (the index list, then the voxel it names), and a workgroup has one wave per SIMD to hide them with.  An inlier past the
// row's n_pl >= 1 is clamped to the last one: callers ignore it, or do not mind a repeat.
constexpr int PRISM_ROWS = 4;
template <int R>
__device__ __forceinline__ void load_inliers(const float4* PP, const int* PI, int first, int n_pl, int N, float4 (&p)[R]) {
    int e[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = min(first + j * BLOCK, n_pl - 1);
        e[j] = PI ? min(max(PI[i], 0), N - 1) : i;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) p[j] = PP[e[j]];
}

__global__ void __launch_bounds__(BLOCK) k_prism(PrismArgs a) {
    __shared__ PrismPoint s_pts[PRISM_LDS_POINTS];
    __shared__ int32_t s_hull[2 * PRISM_MAX_HULL];
    __shared__ long long s_key[WAVES_PER_BLOCK][8];
    __shared__ PrismPoint s_best[2][WAVES_PER_BLOCK];
    __shared__ int s_valid[2][WAVES_PER_BLOCK];
    __shared__ int s_cnt[WAVES_PER_BLOCK];
    __shared__ int s_nsurv;
    __shared__ int s_class[4];
    const int f = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = a.N;
    const size_t fbase = (size_t)f * N;
    const int hv = a.have ? a.have[f] : 1;
    const int n = min(min(max(a.fs[f].n_o, 0), N), a.mpitch);
    const int n_pl = hv ? min(max(a.fs[f].n_plane, 0), N) : 0;
    const float4 m = a.model[f];
    const PrismPlane P = prism_plane(hv ? m.x : 0.f, hv ? m.y : 0.f, hv ? m.z : 0.f, hv ? m.w : 0.f);
    const float4* PP = a.plane_pts + fbase;
    const int* PI = a.plane_idx ? a.plane_idx + fbase : nullptr;
    PrismPoint* G = reinterpret_cast<PrismPoint*>(a.scratch) + fbase;
    if (threadIdx.x == 0) { s_nsurv = 0; s_class[0] = s_class[1] = s_class[2] = s_class[3] = 0; }

    // ---- A: the extremes in eight directions
    long long key[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) key[d] = PRISM_NO_KEY;
    for (int i0 = threadIdx.x; i0 < n_pl; i0 += PRISM_ROWS * BLOCK) {
        float4 p[PRISM_ROWS];
        load_inliers<PRISM_ROWS>(PP, PI, i0, n_pl, N, p);
#pragma unroll
        for (int j = 0; j < PRISM_ROWS; ++j) {   // (a clamped repeat of the last inlier changes no maximum)
            double h;
            int32_t u, v;
            prism_project(P, p[j].x, p[j].y, p[j].z, &h, &u, &v);
            key[0] = max(key[0], prism_key(-u, -v));
            key[1] = max(key[1], prism_key(-u - v, -u));
            key[2] = max(key[2], prism_key(-v, u));
            key[3] = max(key[3], prism_key(u - v, u));
            key[4] = max(key[4], prism_key(u, v));
            key[5] = max(key[5], prism_key(u + v, u));
            key[6] = max(key[6], prism_key(v, -u));
            key[7] = max(key[7], prism_key(v - u, -u));
        }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key[d] = max(key[d], __shfl_xor(key[d], o, WAVE));
        if (lane == 0) s_key[w][d] = key[d];
    }
    __syncthreads();
    PrismPoint E[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        long long k = s_key[0][d];
        for (int q = 1; q < WAVES_PER_BLOCK; ++q) k = max(k, s_key[q][d]);
        key[d] = n_pl > 0 ? k : prism_key(0, 0);   // (no inlier: the eight are never read, but decode something defined)
    }
    {
        const int32_t w0 = prism_key_w(key[0]), t0 = prism_key_t(key[0]), w1 = prism_key_w(key[1]), t1 = prism_key_t(key[1]);
        const int32_t w2 = prism_key_w(key[2]), t2 = prism_key_t(key[2]), w3 = prism_key_w(key[3]), t3 = prism_key_t(key[3]);
        const int32_t w4 = prism_key_w(key[4]), t4 = prism_key_t(key[4]), w5 = prism_key_w(key[5]), t5 = prism_key_t(key[5]);
        const int32_t w6 = prism_key_w(key[6]), t6 = prism_key_t(key[6]), w7 = prism_key_w(key[7]), t7 = prism_key_t(key[7]);
        E[0] = PrismPoint{-w0, -t0};
        E[1] = PrismPoint{-t1, -w1 + t1};
        E[2] = PrismPoint{t2, -w2};
        E[3] = PrismPoint{t3, t3 - w3};
        E[4] = PrismPoint{w4, t4};
        E[5] = PrismPoint{t5, w5 - t5};
        E[6] = PrismPoint{-t6, w6};
        E[7] = PrismPoint{-t7, w7 - t7};
    }
    int nedge = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) nedge += (E[d].u != E[(d + 1) & 7].u || E[d].v != E[(d + 1) & 7].v) ? 1 : 0;

    // ---- B: drop what is strictly inside the polygon of the eight; the survivors to LDS and to the row's scratch
    const uint64_t lt = lanemask_lt();
    for (int i0 = 0; i0 < n_pl; i0 += PRISM_ROWS * BLOCK) {   // (the same trip count for every lane: the ballots below are whole)
        const int first = i0 + (int)threadIdx.x;
        float4 p[PRISM_ROWS];
        load_inliers<PRISM_ROWS>(PP, PI, first, n_pl, N, p);
#pragma unroll
        for (int j = 0; j < PRISM_ROWS; ++j) {
            PrismPoint q;
            double h;
            prism_project(P, p[j].x, p[j].y, p[j].z, &h, &q.u, &q.v);
            bool strict = nedge > 0;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const PrismPoint A = E[d], B = E[(d + 1) & 7];
                if (A.u != B.u || A.v != B.v) strict = strict && prism_cross(A.u, A.v, B.u, B.v, q.u, q.v) > 0;
            }
            const bool surv = first + j * BLOCK < n_pl && !strict;
            const uint64_t bal = ballot64(surv);
            int base = 0;
            if (lane == 0 && bal) base = atomicAdd(&s_nsurv, __popcll(bal));
            base = __shfl(base, 0, WAVE);
            if (surv) {
                const int slot = base + __popcll(bal & lt);   // (< n_pl <= N: inside the row's scratch)
                G[slot] = q;
                if (slot < PRISM_LDS_POINTS) s_pts[slot] = q;
            }
        }
    }
    __syncthreads();
    const int ns = min(s_nsurv, n_pl);
    const bool in_lds = ns <= PRISM_LDS_POINTS;

    // ---- C: the march
    int nh = 0, overflow = 0;
    if (ns > 0) {
        PrismPoint cur = E[0];
        const PrismPoint start = cur;
        if (threadIdx.x == 0) { s_hull[0] = cur.u; s_hull[1] = cur.v; }
        nh = 1;
        for (int step = 0; step <= PRISM_MAX_HULL; ++step) {
            PrismPoint best = {0, 0};
            bool valid = false;
            for (int j = threadIdx.x; j < ns; j += BLOCK) {
                const PrismPoint q = in_lds ? s_pts[j] : G[j];
                if (q.u == cur.u && q.v == cur.v) continue;
                if (!valid || prism_better(cur, best, q)) { best = q; valid = true; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                PrismPoint q;
                q.u = __shfl_xor(best.u, o, WAVE);
                q.v = __shfl_xor(best.v, o, WAVE);
                const bool qvalid = __shfl_xor((int)valid, o, WAVE) != 0;
                if (qvalid && (!valid || prism_better(cur, best, q))) { best = q; valid = true; }
            }
            const int buf = step & 1;   // (two buffers: one barrier per vertex)
            if (lane == 0) { s_best[buf][w] = best; s_valid[buf][w] = valid ? 1 : 0; }
            __syncthreads();
            valid = false;
            for (int q = 0; q < WAVES_PER_BLOCK; ++q) {
                const PrismPoint c = s_best[buf][q];
                if (s_valid[buf][q] && (!valid || prism_better(cur, best, c))) { best = c; valid = true; }
            }
            if (!valid || (best.u == start.u && best.v == start.v)) break;   // all points are one; or the hull is closed
            if (nh == PRISM_MAX_HULL) { overflow = 1; break; }
            if (threadIdx.x == 0) { s_hull[2 * nh] = best.u; s_hull[2 * nh + 1] = best.v; }
            ++nh;
            cur = best;
        }
    }
    if (overflow) nh = 0;
    __syncthreads();
    if (a.hull)
        for (int i = threadIdx.x; i < 2 * nh; i += BLOCK) a.hull[(size_t)f * 2 * PRISM_MAX_HULL + i] = s_hull[i];

    // ---- D: step 7 and the ordered compaction
    const float4* Q = a.pts + fbase;
    int cls_n[4] = {0, 0, 0, 0};
    int out0 = 0;
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int base = t0 + w * WAVE_SPAN + lane;
        float4 p[ITEMS];
        uint64_t bal[ITEMS];
        load_rows_clamped<ITEMS>(Q, base, n, p);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            bool keep = false;
            if (base + j * WAVE < n) {
                int cls = PRISM_KEPT;
                if (hv) {
                    double h;
                    int32_t u, v;
                    prism_project(P, p[j].x, p[j].y, p[j].z, &h, &u, &v);
                    cls = prism_classify(h, u, v, a.hmin, a.hmax, s_hull, nh);
                    cls_n[1] += cls == PRISM_BELOW; cls_n[2] += cls == PRISM_ABOVE; cls_n[3] += cls == PRISM_OUTSIDE;
                }
                keep = cls == PRISM_KEPT;
            }
            bal[j] = ballot64(keep);
        }
        int tot;
        int pos = out0 + tile_prefix<ITEMS>(bal, s_cnt, &tot);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int e = base + j * WAVE, r = pos + __popcll(bal[j] & lt);   // (r <= e < n: inside the row)
            const bool keep = (bal[j] >> lane) & 1ull;
            if (keep) {
                if (a.out) a.out[fbase + r] = p[j];
                if (a.kept_idx) a.kept_idx[fbase + r] = e;
            }
            if (e < n) a.map[(size_t)f * a.mpitch + e] = keep ? r : -1;
            pos += __popcll(bal[j]);
        }
        out0 += tot;
    }
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const int s = wave_sum_i32(cls_n[k]);
        if (lane == 0 && s) atomicAdd(&s_class[k], s);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PrismRecord r;
        r.n_before = n; r.n_kept = out0; r.n_below = s_class[1]; r.n_above = s_class[2]; r.n_outside = s_class[3];
        r.hull_vertices = nh; r.axis_u = hv ? P.k1 : 0; r.axis_v = hv ? P.k2 : 0; r.overflow = overflow;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        a.rec[f] = r;
        // the label calls (rule C15) take the map with a record in the outlier filter's form: they read n_before
        OutlierRecord lr;
        lr.n_before = n; lr.n_finite = n; lr.n_kept = out0; lr.computed = 0;
        lr.mean = lr.stddev = lr.threshold = 0.0;
        a.lrec[f] = lr;
        a.fs[f].n_o = out0;
        if (a.mirror) a.mirror[f].n_o = out0;
    }
}

// With the outlier filter behind the prism, the map the label calls take is the composition: S3 index -> prism -> filter.
__global__ void __launch_bounds__(BLOCK) k_prism_compose_map(int* __restrict__ pmap, const OutlierRecord* __restrict__ lrec, const int* __restrict__ omap,
                                                             int pitch) {
    const int f = blockIdx.y;
    const int n = min(max(lrec[f].n_before, 0), pitch);
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    const int r = pmap[(size_t)f * pitch + e];
    pmap[(size_t)f * pitch + e] = r >= 0 && r < pitch ? omap[(size_t)f * pitch + r] : -1;
}

// ---- host launchers --------------------------------------------------------------------------------------------------------------
void launch_prism(hipStream_t s, int F, const PrismArgs& a) {
    if (F <= 0) return;
    hipLaunchKernelGGL(k_prism, dim3((unsigned)F), dim3(BLOCK), 0, s, a);
}
void launch_prism_compose_map(hipStream_t s, int F, int* pmap, const OutlierRecord* lrec, const int* omap, int pitch) {
    if (F <= 0 || pitch <= 0) return;
    hipLaunchKernelGGL(k_prism_compose_map, dim3((unsigned)((pitch + BLOCK - 1) / BLOCK), (unsigned)F), dim3(BLOCK), 0, s, pmap, lrec, omap, pitch);
}

}  // namespace cd
