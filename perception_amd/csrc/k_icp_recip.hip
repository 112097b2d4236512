// k_icp_recip.hip - S6 with canonical rule C22 (perception_amd/icp_reciprocal.py is the specification): reciprocal
// correspondences, opt-in through cd_set_icp_reciprocal.
//
// The mode's driver (icp_run_sliced, icp_stage.hip) is the sliced multi-launch loop with these two kernels behind every
// k_icp_iter<true>: the iteration kernel has moved the cluster's points in d_src to the positions X its search used (a cluster that
// finished in this launch got its last transformation instead, and is skipped here), left every point's neighbour (position in the
// k-d patch order) and float d2 in d_nn / d_d2, indexed per point, and its own moment sums and count in the iteration's slot.
//   k_icp_recip_flags(it): the reverse test.  A workgroup of 256 threads takes RC_CHUNK consecutive points of one live, unfinished
//     cluster as queries - each lane up to RC_ROWS of them, the query being the point's template point tplk[nn[i]] - and passes ALL
//     the cluster's points through LDS in tiles of RC_TILE float4 (8 KiB), padded with +inf points to a multiple of 8 - the scan
//     of allpairs_scan.hpp, which k_pair_score shares.  The loop reads target e for all lanes at once (one address: a broadcast
//     ds_read_b128) and this kernel's update keeps two running minima per row: over the sources before the row's own index and
//     over those from it on.  Tiles and chunks are aligned alike, so a tile lies wholly
//     before the chunk, wholly behind it, or is the chunk itself - only that one compares indices per pair.  A point of K0 is kept
//     iff recip_keep(before, from, own); the flag of every point of the chunk goes to d_rkeep with a plain byte store.  A query's
//     minima are complete inside one workgroup, minima do not depend on the order of the targets, and nothing but the flags
//     leaves a workgroup: the result does not depend on how the cluster is split.
//   k_icp_recip_fold(it): one workgroup per cluster, k_icp_reject's steps c and d (icp_kept_fold.hpp has them for both):
//     moment_terms of every flagged correspondence, added per lane as 64-bit integers, folded per wave (wave_fold_to_lds) and per
//     workgroup (ds_add_u64); then plain vector stores REPLACE the slot's 16 sums (d_acc[cluster * 3 + it % 3]) and count
//     (d_ncorr), which k_icp_solve<true>(it + 1) reads, and update the stats record.  Its own: the count of K0, with fewer than
//     three points in which the slot's count is |K0|, and last_n0.
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
#include "allpairs_scan.hpp"
#include "common.hpp"
#include "icp_kept_fold.hpp"
#include "icp_recip_math.hpp"
#include "kernels.hpp"

namespace cd {

constexpr int RC_THREADS = 256;
constexpr int RC_ROWS = 2;                       // queries per lane at the most
constexpr int RC_CHUNK = RC_ROWS * RC_THREADS;   // queries of a workgroup
constexpr int RC_TILE = 512;                     // targets per LDS tile
static_assert(RC_TILE == RC_CHUNK, "a tile is before the chunk, behind it, or the chunk itself");
static_assert(RC_TILE % 8 == 0 && RC_TILE % RC_THREADS == 0, "the tile is padded to a multiple of 8 and loaded by whole workgroups");

__global__ void __launch_bounds__(RC_THREADS)
k_icp_recip_flags(int it, const IcpCluster* __restrict__ cl, const IcpState* __restrict__ st, const float4* __restrict__ src,
                  const float4* __restrict__ tplk, const int* __restrict__ nn, const float* __restrict__ d2buf, float d2_max, uint8_t* __restrict__ keep) {
    __shared__ float4 s_tile[RC_TILE];
    const int k = blockIdx.x;
    const IcpCluster c = cl[k];
    const int q0 = (int)blockIdx.y * RC_CHUNK;
    if (q0 >= c.n || kept_skips(c, st, k, it)) return;   // (the whole workgroup)
    const int qn = min(RC_CHUNK, c.n - q0);
    const float4* __restrict__ pts = src + c.src_off;
    const int* __restrict__ nnp = nn + c.src_off;
    const float4* __restrict__ tp = tplk + c.tpl_off;
    // the queries (a lane beyond the range holds a copy of the range's last query and writes nothing)
    float qx[RC_ROWS], qy[RC_ROWS], qz[RC_ROWS], own[RC_ROWS], before[RC_ROWS], from[RC_ROWS];
    int li[RC_ROWS];
#pragma unroll
    for (int j = 0; j < RC_ROWS; ++j) {
        li[j] = scan_clamp(scan_row<RC_THREADS>(j), qn);
        const float4 p = pts[q0 + li[j]];
        const float4 q = tp[min(max(nnp[q0 + li[j]], 0), c.tpl_m - 1)];   // (a position k_icp_iter wrote; the clamp keeps a read inside the template)
        qx[j] = q.x; qy[j] = q.y; qz[j] = q.z;
        own[j] = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
        before[j] = INFINITY; from[j] = INFINITY;
    }
    const int rows = scan_live_rows<RC_THREADS>(qn);
    // the targets: every point of the cluster, tile by tile.  Tiles and chunks are aligned alike (RC_TILE == RC_CHUNK): a tile
    // lies wholly before the chunk, wholly behind it, or is the chunk itself, and only that one compares indices - a row's index
    // inside the chunk, li[j], is then its index inside the tile.
    for (int t0 = 0; t0 < c.n; t0 += RC_TILE) {
        const int cnt8 = scan_load_tile<RC_THREADS>(s_tile, pts, t0, min(RC_TILE, c.n - t0));
        __syncthreads();
        if (t0 < q0) scan_tile_rows<RC_ROWS>(rows, s_tile, cnt8, qx, qy, qz, [&](int j, int, float d) { before[j] = recip_min(before[j], d); });
        else if (t0 > q0) scan_tile_rows<RC_ROWS>(rows, s_tile, cnt8, qx, qy, qz, [&](int j, int, float d) { from[j] = recip_min(from[j], d); });
        else scan_tile_rows<RC_ROWS>(rows, s_tile, cnt8, qx, qy, qz, [&](int j, int e, float d) {
            const bool b = e < li[j];
            before[j] = recip_min(before[j], b ? d : INFINITY);
            from[j] = recip_min(from[j], b ? INFINITY : d);
        });
        __syncthreads();
    }
    const float* __restrict__ d2 = d2buf + c.src_off;
    uint8_t* __restrict__ kp = keep + c.src_off;
#pragma unroll
    for (int j = 0; j < RC_ROWS; ++j) {
        const int r = scan_row<RC_THREADS>(j);
        if (r < qn) kp[q0 + r] = icp_in_k0(d2[q0 + r], d2_max) && recip_keep(before[j], from[j], own[j]) ? 1 : 0;
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
    if (kept_skips(c, st, k, it)) return;
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
        if (icp_in_k0(v, bnd.d2_max)) ++n0;
        if (!kp[i]) continue;
        kept_add(pts, nnp, tp, c.tpl_m, i, v, S);
        ++kept;
    }
    wave_fold_to_lds(S, 16, s_sum);
    n0 = wave_sum_i32(n0);
    kept = wave_sum_i32(kept);
    if (lane == 0 && n0) atomicAdd(&s_cnt[0], (uint32_t)n0);
    if (lane == 0 && kept) atomicAdd(&s_cnt[1], (uint32_t)kept);
    __syncthreads();
    // the iteration's slot and the record
    const size_t slot = kept_store_sums(acc, s_sum, k, it);
    if (tid == 16) {
        const int k0 = (int)s_cnt[0];
        const int n = k0 < ICP_MIN_CORR ? k0 : (int)s_cnt[1];   // (step 1: nothing is tested, K0 itself is what is left)
        bnd.ncorr[slot] = (uint32_t)n;
        RecipStats rs = rstat[k];
        kept_update(rs.kept, it, n);
        rs.last_n0 = k0;
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
