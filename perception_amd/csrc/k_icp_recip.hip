// k_icp_recip.hip - S6 with canonical rule C22 (perception_amd/icp_reciprocal.py is the specification): reciprocal
// correspondences, opt-in through cd_set_icp_reciprocal.
//
// The mode's driver (icp_run_sliced, icp_stage.hip) is the sliced multi-launch loop with these two kernels behind every
// k_icp_iter<true>: the iteration kernel has moved the cluster's points in d_src to the positions X its search used (a cluster that
// finished in this launch got its last transformation instead, and is skipped here), left every point's neighbour (position in the
// k-d patch order) and float d2 in d_nn / d_d2, indexed per point, and its own moment sums and count in the iteration's slot.
//   k_icp_recip_flags(it): the reverse test.  A workgroup of 256 threads takes RC_CHUNK consecutive points of one live, unfinished
//     cluster as queries - each lane up to RC_ROWS of them, the query being the point's template point tplk[nn[i]] - and passes ALL
//     the cluster's points through LDS in tiles of RC_TILE float4 (8 KiB), padded with +inf points to a multiple of 8.  The loop
//     reads target e for all lanes at once (one address: a broadcast ds_read_b128) and updates two running minima per row: over
//     the sources before the row's own index and over those from it on.  Tiles and chunks are aligned alike, so a tile lies wholly
//     before the chunk, wholly behind it, or is the chunk itself - only that one compares indices per pair.  A point of K0 is kept
//     iff recip_keep(before, from, own); the flag of every point of the chunk goes to d_rkeep with a plain byte store.  A query's
//     minima are complete inside one workgroup, minima do not depend on the order of the targets, and nothing but the flags
//     leaves a workgroup: the result does not depend on how the cluster is split.
//   k_icp_recip_fold(it): one workgroup per cluster, as k_icp_reject's steps c and d: moment_terms of every flagged
//     correspondence, added per lane as 64-bit integers, folded per wave (wave_fold_to_lds) and per workgroup (ds_add_u64); then
//     plain vector stores REPLACE the slot's 16 sums (d_acc[cluster * 3 + it % 3]) and count (d_ncorr), which
//     k_icp_solve<true>(it + 1) reads, and update the stats record.  With fewer than three points in K0 the count is |K0|.
// No other kernel changes.  At most n^2 pair tests per cluster and iteration: eight f32 operations and half a v_min3_f32 each (the
// compiler pairs the minima of two targets), two compares and selects more in the chunk's own tile.
//
// Two queries a lane, not k_pair_score's four: a batch's clusters finish at different iterations, most launches find few of them
// left, and then a launch lasts as long as one workgroup - with four rows the bench batch's ICP stage took 29 ms, with two 24 ms.
//
// Budget (compiler's report, gfx950): k_icp_recip_flags LDS 8192 B, 76 VGPRs (the loop is unrolled over eight targets), 64 SGPRs,
// no scratch - six waves a SIMD, six workgroups a CU by registers; LDS would allow twenty.  k_icp_recip_fold LDS 136 B, 76 VGPRs
// (16 running sums and 16 terms as 64-bit pairs), 50 SGPRs, no scratch - six waves a SIMD.  No MFMA: nothing here is a
// contraction.
#include "common.hpp"
#include "icp_recip_math.hpp"
#include "icp_solve.hpp"
#include "kernels.hpp"

namespace cd {

constexpr int RC_THREADS = 256;
constexpr int RC_ROWS = 2;                       // queries per lane at the most
constexpr int RC_CHUNK = RC_ROWS * RC_THREADS;   // queries of a workgroup
constexpr int RC_TILE = 512;                     // targets per LDS tile
static_assert(RC_TILE == RC_CHUNK, "a tile is before the chunk, behind it, or the chunk itself");
static_assert(RC_TILE % 8 == 0 && RC_TILE % RC_THREADS == 0, "the tile is padded to a multiple of 8 and loaded by whole workgroups");

enum { RC_BEFORE = 0, RC_FROM = 1, RC_DIAG = 2 };

// One tile against the lane's rows.  li[j]: the row's index inside the chunk (= inside the tile, RC_DIAG).
template <int ROWS, int MODE>
__device__ __forceinline__ void recip_scan_tile(const float4* __restrict__ tile, int cnt8, const float (&qx)[RC_ROWS], const float (&qy)[RC_ROWS],
                                                const float (&qz)[RC_ROWS], const int (&li)[RC_ROWS], float (&before)[RC_ROWS], float (&from)[RC_ROWS]) {
#pragma unroll 8
    for (int e = 0; e < cnt8; ++e) {
        const float4 g = tile[e];   // (the same address in every lane)
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const float d = recip_d2(qx[j], qy[j], qz[j], g.x, g.y, g.z);
            if (MODE == RC_BEFORE) before[j] = recip_min(before[j], d);
            else if (MODE == RC_FROM) from[j] = recip_min(from[j], d);
            else {
                const bool b = e < li[j];
                before[j] = recip_min(before[j], b ? d : INFINITY);
                from[j] = recip_min(from[j], b ? INFINITY : d);
            }
        }
    }
}

template <int MODE>
__device__ __forceinline__ void recip_scan_rows(int rows, const float4* __restrict__ tile, int cnt8, const float (&qx)[RC_ROWS], const float (&qy)[RC_ROWS],
                                                const float (&qz)[RC_ROWS], const int (&li)[RC_ROWS], float (&before)[RC_ROWS], float (&from)[RC_ROWS]) {
    static_assert(RC_ROWS == 2, "one instantiation per number of live rows");
    if (rows == 1) recip_scan_tile<1, MODE>(tile, cnt8, qx, qy, qz, li, before, from);
    else recip_scan_tile<2, MODE>(tile, cnt8, qx, qy, qz, li, before, from);
}

// a cluster the kernels of launch `it` leave alone: pre-marked, or finished (k_icp_solve(it) has run)
__device__ __forceinline__ bool recip_skips(const IcpCluster& c, const IcpState* __restrict__ st, int k, int it) {
    if (c.n < RECIP_MIN_CORR || c.tpl_m <= 0) return true;
    return st[(size_t)k * 2 + (it & 1)].done || st[(size_t)k * 2 + ((it + 1) & 1)].done;
}

__global__ void __launch_bounds__(RC_THREADS)
k_icp_recip_flags(int it, const IcpCluster* __restrict__ cl, const IcpState* __restrict__ st, const float4* __restrict__ src,
                  const float4* __restrict__ tplk, const int* __restrict__ nn, const float* __restrict__ d2buf, float d2_max, uint8_t* __restrict__ keep) {
    __shared__ float4 s_tile[RC_TILE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const IcpCluster c = cl[k];
    const int q0 = (int)blockIdx.y * RC_CHUNK;
    if (q0 >= c.n || recip_skips(c, st, k, it)) return;   // (the whole workgroup)
    const int qn = min(RC_CHUNK, c.n - q0);
    const float4* __restrict__ pts = src + c.src_off;
    const int* __restrict__ nnp = nn + c.src_off;
    const float4* __restrict__ tp = tplk + c.tpl_off;
    // the queries (a lane beyond the range holds a copy of the range's last query and writes nothing)
    float qx[RC_ROWS], qy[RC_ROWS], qz[RC_ROWS], own[RC_ROWS], before[RC_ROWS], from[RC_ROWS];
    int li[RC_ROWS];
#pragma unroll
    for (int j = 0; j < RC_ROWS; ++j) {
        const int r = j * RC_THREADS + tid;
        li[j] = r < qn ? r : qn - 1;
        const float4 p = pts[q0 + li[j]];
        const float4 q = tp[min(max(nnp[q0 + li[j]], 0), c.tpl_m - 1)];   // (a position k_icp_iter wrote; the clamp keeps a read inside the template)
        qx[j] = q.x; qy[j] = q.y; qz[j] = q.z;
        own[j] = recip_d2(q.x, q.y, q.z, p.x, p.y, p.z);
        before[j] = INFINITY; from[j] = INFINITY;
    }
    const int rows = (qn + RC_THREADS - 1) / RC_THREADS;
    // the targets: every point of the cluster, tile by tile
    for (int t0 = 0; t0 < c.n; t0 += RC_TILE) {
        const int cnt = min(RC_TILE, c.n - t0), cnt8 = (cnt + 7) & ~7;
        for (int e = tid; e < cnt8; e += RC_THREADS) {
            float4 g = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            if (e < cnt) { const float4 p = pts[t0 + e]; g = make_float4(p.x, p.y, p.z, 0.f); }
            s_tile[e] = g;
        }
        __syncthreads();
        if (t0 < q0) recip_scan_rows<RC_BEFORE>(rows, s_tile, cnt8, qx, qy, qz, li, before, from);
        else if (t0 > q0) recip_scan_rows<RC_FROM>(rows, s_tile, cnt8, qx, qy, qz, li, before, from);
        else recip_scan_rows<RC_DIAG>(rows, s_tile, cnt8, qx, qy, qz, li, before, from);
        __syncthreads();
    }
    const float* __restrict__ d2 = d2buf + c.src_off;
    uint8_t* __restrict__ kp = keep + c.src_off;
#pragma unroll
    for (int j = 0; j < RC_ROWS; ++j) {
        const int r = j * RC_THREADS + tid;
        if (r < qn) kp[q0 + r] = recip_in_k0(d2[q0 + r], d2_max) && recip_keep(before[j], from[j], own[j]) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(RC_THREADS)
k_icp_recip_fold(int it, const IcpCluster* __restrict__ cl, const IcpState* __restrict__ st, const float4* __restrict__ src,
                 const float4* __restrict__ tplk, const int* __restrict__ nn, const float* __restrict__ d2buf, const uint8_t* __restrict__ keep,
                 unsigned long long* __restrict__ acc, IcpBound bnd, RecipStats* __restrict__ rstat) {
    __shared__ unsigned long long s_sum[16];
    __shared__ uint32_t s_cnt[2];   // |K0|, flagged
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const IcpCluster c = cl[k];
    if (recip_skips(c, st, k, it)) return;
    if (tid < 16) s_sum[tid] = 0ull;
    if (tid >= 16 && tid < 18) s_cnt[tid - 16] = 0u;
    __syncthreads();
    unsigned long long S[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) S[j] = 0ull;
    int n0 = 0, kept = 0;
    const float4* pts = src + c.src_off;
    const int* nnp = nn + c.src_off;
    const float* d2 = d2buf + c.src_off;
    const uint8_t* kp = keep + c.src_off;
    const float4* tp = tplk + c.tpl_off;
    for (int i = tid; i < c.n; i += RC_THREADS) {
        const float v = d2[i];
        if (recip_in_k0(v, bnd.d2_max)) ++n0;
        if (!kp[i]) continue;
        const float4 p = pts[i];
        const float4 q = tp[min(max(nnp[i], 0), c.tpl_m - 1)];
        const float pv[3] = {p.x, p.y, p.z}, qv[3] = {q.x, q.y, q.z};
        unsigned long long t[16];
        moment_terms(pv, qv, v, t);
#pragma unroll
        for (int a = 0; a < 16; ++a) S[a] += t[a];
        ++kept;
    }
    wave_fold_to_lds(S, 16, s_sum);
    n0 = wave_sum_i32(n0);
    kept = wave_sum_i32(kept);
    if (lane == 0 && n0) atomicAdd(&s_cnt[0], (uint32_t)n0);
    if (lane == 0 && kept) atomicAdd(&s_cnt[1], (uint32_t)kept);
    __syncthreads();
    // the iteration's slot and the record
    const size_t slot = (size_t)k * 3 + (size_t)(it % 3);
    if (tid < 16) acc[slot * 16 + tid] = s_sum[tid];
    if (tid == 16) {
        const int k0 = (int)s_cnt[0];
        const int n = k0 < RECIP_MIN_CORR ? k0 : (int)s_cnt[1];   // (step 1: nothing is tested, K0 itself is what is left)
        bnd.ncorr[slot] = (uint32_t)n;
        RecipStats rs = rstat[k];
        if (it == 0) { rs.first_kept = n; rs.min_kept = n; }
        else rs.min_kept = min(rs.min_kept, n);
        rs.last_kept = n;
        rs.last_n0 = k0;
        if (n < RECIP_MIN_CORR) rs.stopped_few = 1;
        rstat[k] = rs;
    }
}

void launch_icp_recip(hipStream_t s, int it, int ncl, int max_n, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, const IcpBound& bnd,
                      uint8_t* keep, RecipStats* rstat) {
    if (ncl <= 0 || max_n <= 0) return;
    const int chunks = (max_n + RC_CHUNK - 1) / RC_CHUNK;
    hipLaunchKernelGGL(k_icp_recip_flags, dim3(ncl, chunks), dim3(RC_THREADS), 0, s, it, P.cl, P.st, S.src, T.tplk, S.nn, S.d2, bnd.d2_max, keep);
    hipLaunchKernelGGL(k_icp_recip_fold, dim3(ncl), dim3(RC_THREADS), 0, s, it, P.cl, P.st, S.src, T.tplk, S.nn, S.d2, keep, S.acc, bnd, rstat);
}

}  // namespace cd
