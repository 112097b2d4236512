// k_outlier.hip - canonical rule C16: statistical outlier removal on a cloud (outlier_math.hpp holds the arithmetic,
// perception_amd/outlier_filter.py the specification).
//
// Two kernels on the context's stream, over rows of `N` points (a frame's object cloud, or the one cloud of cd_outlier_filter):
//   1. k_outlier_knn     dist_i of every point.  One wave per query at a time, OUT_QPW queries per wave and OUT_QPB per
//                        workgroup; the row's points pass through LDS in tiles of OUT_TILE candidates (a non-finite point is
//                        staged with an all-ones mask word that turns its key into "no candidate"), each tile read by all the
//                        workgroup's queries.  A wave takes 64 candidates per step and keeps the 64 smallest keys seen so far
//                        sorted ascending across its lanes (non-negative floats order as their bit patterns).  One ballot skips
//                        a step that holds nothing below the current (mean_k + 1)-th; a step with a few such candidates inserts them
//                        one at a time (a lane shift and a select each); a step with many sorts its 64 keys descending in a bitonic
//                        network, takes the lower half min(best[i], step[i]) and sorts it with the six stages of a bitonic
//                        merge.  Lane order is then the ascending order step 4 of the rule needs: lane 0 is the query itself.
//   2. k_outlier_select  one workgroup per row.  Lane 0 runs the two sequential double sums of step 5 over the row's dist
//                        (staged through LDS by the whole workgroup) and leaves the row's OutlierRecord; then the workgroup
//                        walks the row tile by tile, decides step 6 and compacts the kept points in order - whole float4
//                        records - with the running count carried in order: no atomics, no chained scan.  It also writes the
//                        map (index in the filtered row, or -1), the kept indices and the row's new count.
// Flags, the tile scan and a scatter behind the statistics would be three more launches.  The statistics kernel is one workgroup
// per row already and bound by its chain of double additions; a row has a few thousand points, so the same workgroup compacts
// its two tiles in less time than three more launches take to start.
//
// Every count read from memory is clamped to the row it indexes before it bounds a loop, every index is below that count, and a
// row with no points or no more than mean_k finite points passes through untouched.
#include <algorithm>

#include "kernels.hpp"
#include "outlier_math.hpp"

namespace cd {

constexpr int OUT_TILE = CD_OUTLIER_LDS_TILE;          // candidates staged at a time: 16 KiB
constexpr int OUT_QPW = 4;                             // queries a wave carries through every tile
constexpr int OUT_QPB = WAVES_PER_BLOCK * OUT_QPW;     // per workgroup: a tile is staged once for 16 queries
constexpr int OUT_INSERT_MAX = 12;                     // candidates of a step that are still inserted one at a time
constexpr int OUT_DCHUNK = 2048;                       // dist values staged for lane 0's sequential sums
static_assert(OUT_TILE % WAVE == 0 && OUT_TILE % BLOCK == 0, "whole steps, whole staging rounds");
static_assert(OUT_TILE % OUT_QPB == 0, "a workgroup's queries lie in one tile");
static_assert(OUTLIER_MAX_K + 1 <= WAVE, "the mean_k + 1 best keys of a query: one per lane");

// keys sorted ascending across the lanes; v goes in at its place, the keys above it move one lane up (lane 63's leaves).
// The lane to the left through the DPP path (wave_shr:1; lane 0 reads the `old` operand, 0): no LDS crossbar, no address register.
__device__ __forceinline__ uint32_t outlier_insert(uint32_t best, uint32_t v) {
    const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)best, 0x138, 0xf, 0xf, false);
    return best <= v ? best : max(v, up);
}

// the 64 smallest of best (ascending across the lanes) and key (any order), ascending across the lanes
__device__ __noinline__ uint32_t outlier_merge(uint32_t best, uint32_t key, int lane) {
    // bitonic sort of key, DESCENDING
#pragma unroll
    for (int k = 2; k <= WAVE; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t p = (uint32_t)__shfl_xor((int)key, j, WAVE);
            const bool down = (lane & k) == 0 || k == WAVE;       // this block of k lanes ends up descending
            const bool first = (lane & j) == 0;                   // the lower lane of the pair
            key = (first == down) ? max(key, p) : min(key, p);
        }
    }
    // best ascending, key descending: the elementwise minimum holds the 64 smallest of the 128, as a bitonic sequence
    best = min(best, key);
#pragma unroll
    for (int j = WAVE >> 1; j > 0; j >>= 1) {
        const uint32_t p = (uint32_t)__shfl_xor((int)best, j, WAVE);
        best = (lane & j) == 0 ? min(best, p) : max(best, p);
    }
    return best;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_outlier_knn(const float4* __restrict__ pts, int N, const FrameState* __restrict__ fs, int mean_k,
                                                       float* __restrict__ dist, int dpitch) {
    __shared__ float4 s_pt[OUT_TILE];
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = min(min(max(fs[f].n_o, 0), N), dpitch);
    mean_k = min(max(mean_k, 1), OUTLIER_MAX_K);   // (the host checks it: the lane it names exists whatever comes in)
    const int q0 = blockIdx.x * OUT_QPB + w * OUT_QPW;
    if ((int)(blockIdx.x * OUT_QPB) >= n) return;   // (the whole workgroup: before any barrier)
    const float4* P = pts + (size_t)f * N;
    float qx[OUT_QPW], qy[OUT_QPW], qz[OUT_QPW];
    bool live[OUT_QPW];
    uint32_t best[OUT_QPW];
#pragma unroll
    for (int j = 0; j < OUT_QPW; ++j) {
        const float4 q = P[min(q0 + j, n - 1)];
        qx[j] = q.x; qy[j] = q.y; qz[j] = q.z;
        live[j] = q0 + j < n && outlier_finite(q.x, q.y, q.z);
        best[j] = OUTLIER_NO_KEY;
    }
    // The tiles in a ring that starts at the one holding the workgroup's queries, and inside it the steps in a ring that starts
    // at the query's own: the object cloud is in voxel order, so a point's neighbours in the cloud are neighbours in space, the
    // bound drops to nearly its final value within a step or two and most other steps are skipped.  The rule's result is a
    // multiset: it does not depend on the order of the visits.
    const int ntiles = (n + OUT_TILE - 1) / OUT_TILE;
    const int home = (int)(blockIdx.x * OUT_QPB) / OUT_TILE;
    for (int it = 0; it < ntiles; ++it) {
        const int t0 = (home + it < ntiles ? home + it : home + it - ntiles) * OUT_TILE;
        __syncthreads();   // (the previous tile's readers are done)
#pragma unroll
        for (int i = threadIdx.x; i < OUT_TILE; i += BLOCK) {
            const int e = t0 + i;
            float4 p = P[min(e, n - 1)];
            p.w = __uint_as_float(e < n && outlier_finite(p.x, p.y, p.z) ? 0u : OUTLIER_NO_KEY);
            s_pt[i] = p;
        }
        __syncthreads();
        const int steps = (min(OUT_TILE, n - t0) + WAVE - 1) / WAVE;
#pragma unroll
        for (int j = 0; j < OUT_QPW; ++j) {
            if (!live[j]) continue;   // (wave-uniform)
            uint32_t b = best[j];
            // the bound: the (mean_k + 1)-th smallest key so far - a key that is not below it cannot be among the mean_k + 1 best
            uint32_t bound = (uint32_t)__builtin_amdgcn_readlane((int)b, mean_k);
            int s = it == 0 ? min(max((q0 + j - t0) / WAVE, 0), steps - 1) : 0;
            for (int i = 0; i < steps; ++i, s = s + 1 < steps ? s + 1 : 0) {
                const float4 c = s_pt[s * WAVE + lane];
                const uint32_t key = outlier_d2_key(qx[j], qy[j], qz[j], c.x, c.y, c.z) | __float_as_uint(c.w);
                uint64_t mask = ballot64(key < bound);
                if (mask == 0ull) continue;
                if (__popcll(mask) > OUT_INSERT_MAX) {
                    b = outlier_merge(b, key, lane);
                } else {
                    while (mask) {
                        const int src = __ffsll((long long)mask) - 1;
                        mask &= mask - 1ull;
                        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)key, src);
                        if (v < bound) {
                            b = outlier_insert(b, v);
                            bound = (uint32_t)__builtin_amdgcn_readlane((int)b, mean_k);
                        }
                    }
                }
                bound = (uint32_t)__builtin_amdgcn_readlane((int)b, mean_k);
            }
            best[j] = b;
        }
    }
#pragma unroll
    for (int j = 0; j < OUT_QPW; ++j) {
        if (q0 + j >= n) continue;
        float d = 0.0f;
        const uint32_t b = best[j];
        if (live[j] && (uint32_t)__builtin_amdgcn_readlane((int)b, mean_k) != OUTLIER_NO_KEY) {   // (else rule step 2: dist stays 0)
            const uint32_t root = __float_as_uint(outlier_root(b));   // every lane's own key: one square root for the wave
            d = outlier_mean_dist([&](int i) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)root, i)); }, mean_k);
        }
        if (lane == 0) dist[(size_t)f * dpitch + q0 + j] = d;
    }
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_outlier_select(const float4* __restrict__ pts, int N, FrameState* __restrict__ fs, FrameState* __restrict__ mirror,
                                                          const float* __restrict__ dist, int dpitch, int mean_k, double std_mul, int negative,
                                                          float4* __restrict__ out, int* __restrict__ map, int mpitch, int* __restrict__ kept_idx,
                                                          OutlierRecord* __restrict__ rec) {
    __shared__ int s_cnt[WAVES_PER_BLOCK];
    __shared__ float s_d[OUT_DCHUNK];
    __shared__ OutlierRecord s_rec;
    const int f = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(min(min(max(fs[f].n_o, 0), N), dpitch), mpitch);
    const size_t fbase = (size_t)f * N;
    const float4* P = pts + fbase;
    const float* D = dist + (size_t)f * dpitch;
    // the finite points, counted by the workgroup
    int m = 0;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const float4 p = P[i];
        m += outlier_finite(p.x, p.y, p.z) ? 1 : 0;
    }
    m = wave_sum_i32(m);
    if (lane == 0) s_cnt[w] = m;
    __syncthreads();
    m = 0;
    for (int q = 0; q < WAVES_PER_BLOCK; ++q) m += s_cnt[q];
    const int computed = m > mean_k ? 1 : 0;
    // step 5: the sequential sums on one lane, the row's dist staged OUT_DCHUNK values at a time
    OutlierSums sums = {0.0, 0.0};
    if (computed) {
        for (int t0 = 0; t0 < n; t0 += OUT_DCHUNK) {
            const int cnt = min(OUT_DCHUNK, n - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < cnt; i += BLOCK) s_d[i] = D[t0 + i];
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 0; i < cnt; ++i) outlier_accumulate(sums, s_d[i]);
        }
    }
    if (threadIdx.x == 0) {
        s_rec.n_before = n; s_rec.n_finite = m; s_rec.n_kept = 0; s_rec.computed = computed;
        s_rec.mean = s_rec.stddev = s_rec.threshold = 0.0;
        if (computed) outlier_statistics(sums, m, std_mul, &s_rec);
    }
    __syncthreads();
    const double threshold = s_rec.threshold;
    // step 6 and the ordered compaction
    const uint64_t lt = lanemask_lt();
    int out0 = 0;
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int base = t0 + w * WAVE_SPAN + lane;
        float4 p[ITEMS];
        float d[ITEMS];
        uint64_t bal[ITEMS];
        load_rows_clamped<ITEMS>(P, base, n, p);
        load_rows_clamped<ITEMS>(D, base, n, d);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const bool keep = base + j * WAVE < n && outlier_finite(p[j].x, p[j].y, p[j].z) && (!computed || outlier_keep(d[j], threshold, negative));
            bal[j] = ballot64(keep);
        }
        int tot;
        int pos = out0 + tile_prefix<ITEMS>(bal, s_cnt, &tot);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int e = base + j * WAVE, r = pos + __popcll(bal[j] & lt);   // (r <= e < n: inside the row)
            const bool keep = (bal[j] >> lane) & 1ull;
            if (keep) {
                if (out) out[fbase + r] = p[j];
                if (kept_idx) kept_idx[fbase + r] = e;
            }
            if (e < n) map[(size_t)f * mpitch + e] = keep ? r : -1;
            pos += __popcll(bal[j]);
        }
        out0 += tot;
    }
    if (threadIdx.x == 0) {
        s_rec.n_kept = out0;
        rec[f] = s_rec;
        fs[f].n_o = out0;
        if (mirror) mirror[f].n_o = out0;
    }
}

// ---- host launchers --------------------------------------------------------------------------------------------------------------
void launch_outlier_knn(hipStream_t s, const float4* pts, int N, int F, int max_n, const FrameState* fs, int mean_k, float* dist, int dpitch) {
    if (max_n <= 0 || F <= 0) return;
    hipLaunchKernelGGL(k_outlier_knn, dim3((unsigned)((max_n + OUT_QPB - 1) / OUT_QPB), (unsigned)F), dim3(BLOCK), 0, s, pts, N, fs, mean_k, dist, dpitch);
}
void launch_outlier_select(hipStream_t s, const float4* pts, int N, int F, FrameState* fs, FrameState* mirror, const float* dist, int dpitch,
                           int mean_k, double std_mul, int negative, float4* out, int* map, int mpitch, int* kept_idx, OutlierRecord* rec) {
    if (F <= 0) return;
    hipLaunchKernelGGL(k_outlier_select, dim3((unsigned)F), dim3(BLOCK), 0, s, pts, N, fs, mirror, dist, dpitch, mean_k, std_mul, negative, out, map, mpitch,
                       kept_idx, rec);
}

}  // namespace cd
