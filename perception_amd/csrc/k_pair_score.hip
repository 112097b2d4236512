// k_pair_score.hip - canonical rule C21 (perception_amd/pair_score.py is the specification): the two-way registration
// score of (cluster, template) pairs, opt-in through cd_set_pair_score, and the kernel behind cd_pair_score_points.
//
// An exact all-pairs minimum, run in both directions by swapping the roles of the two sets.  A JOB is one direction of one pair:
// its queries and its targets, one of the two being the cluster's points under T (evaluated on the fly by xform_row, once per
// load: the same float32 value wherever it is evaluated), the other the template's.  An ITEM is a range of at most PS_CHUNK queries
// of a job against ALL its targets, so a query's minimum is complete inside one workgroup and nothing but integers crosses
// workgroups: a pair larger than a chunk is split over workgroups by queries only.  The host sorts the items by pair tests,
// largest first; the workgroups of a launch draw them from one queue word.
//
// One workgroup of 256 threads per item at a time (steps a and b are the scan of allpairs_scan.hpp, which k_icp_recip_flags
// shares; the constants, the transform and the update - one minimum per row - are this kernel's):
//   a. every lane loads up to PS_ROWS queries into registers (query base + row * 256 + thread; a lane beyond the range holds a
//      copy of the range's last query and is not counted), each with a running minimum of +inf;
//   b. the targets pass through LDS in tiles of PS_TILE float4 (16 KiB, up to ten workgroups a CU by LDS), padded with +inf
//      points to a multiple of 8; the loop reads target e for all lanes at once - one address, a broadcast ds_read_b128, no bank
//      conflict - and updates the lane's rows: three subtractions, three products, two sums, one v_min_f32 per (query, target) on
//      non-negative values.  The loop is instantiated per number of live rows, so a chunk's empty rows cost nothing;
//   c. the lane's counts and clamped fixq terms (pair_term) are folded by shuffles, per workgroup by LDS atomics, and added to
//      the pair's row of the accumulator with one 64-bit atomic per word: integer sums, order-free.  A non-finite query is counted
//      in the row's PAIR_BAD word, and the host then refuses the pair.
// Budget (compiler's report, gfx950): LDS 16424 B, 109 VGPRs (four rows, the loop unrolled over eight targets), 73 SGPRs, no
// scratch - four waves a SIMD by registers.  No MFMA: nothing here is a contraction.
#include "allpairs_scan.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "pair_score_math.hpp"

namespace cd {

static_assert(PS_CHUNK == PS_ROWS * PS_THREADS, "a chunk is PS_ROWS queries per thread");
static_assert(PS_TILE % 8 == 0 && PS_TILE % PS_THREADS == 0, "the tile is padded to a multiple of 8 and loaded by whole workgroups");

__global__ void __launch_bounds__(PS_THREADS)
k_pair_score(const PairJob* __restrict__ jobs, const PairItem* __restrict__ items, int n_items, const float4* __restrict__ src,
             const float4* __restrict__ tpl, float tau, unsigned long long* __restrict__ acc, int* __restrict__ queue) {
    __shared__ float4 s_tile[PS_TILE];
    __shared__ unsigned long long s_sum[4];   // inside count, inside sum, whole sum, non-finite queries
    __shared__ int s_item;
    const int tid = threadIdx.x, lane = tid & 63;
    for (;;) {
        if (tid == 0) s_item = atomicAdd(queue, 1);
        if (tid < 4) s_sum[tid] = 0ull;
        __syncthreads();
        const int it = s_item;
        if (it >= n_items) return;   // (the whole workgroup)
        const PairItem item = items[it];
        const PairJob job = jobs[item.job];
        const float4* __restrict__ qp = (job.q_src ? src : tpl) + job.q_off;
        const float4* __restrict__ gp = (job.q_src ? tpl : src) + job.g_off;
        // a. the queries
        float qx[PS_ROWS], qy[PS_ROWS], qz[PS_ROWS], best[PS_ROWS];
        int bad = 0;
#pragma unroll
        for (int j = 0; j < PS_ROWS; ++j) {
            const int r = scan_row<PS_THREADS>(j);
            const float4 p = qp[item.q0 + scan_clamp(r, item.qn)];
            if (job.q_src) {
                qx[j] = xform_row(job.T, 0, p.x, p.y, p.z); qy[j] = xform_row(job.T, 1, p.x, p.y, p.z); qz[j] = xform_row(job.T, 2, p.x, p.y, p.z);
            } else { qx[j] = p.x; qy[j] = p.y; qz[j] = p.z; }
            best[j] = INFINITY;
            if (r < item.qn && !pair_finite(qx[j], qy[j], qz[j])) ++bad;
        }
        const int rows = scan_live_rows<PS_THREADS>(item.qn);
        // b. the targets, tile by tile
        for (int t0 = 0; t0 < job.ng; t0 += PS_TILE) {
            const int cnt8 = scan_load_tile<PS_THREADS, true>(s_tile, gp, t0, min(PS_TILE, job.ng - t0), job.q_src, job.T);
            __syncthreads();
            scan_tile_rows<PS_ROWS>(rows, s_tile, cnt8, qx, qy, qz, [&](int j, int, float d) { best[j] = __builtin_fminf(best[j], d); });
            __syncthreads();
        }
        // c. counts and sums
        unsigned long long n_in = 0ull, s_in = 0ull, s_all = 0ull;
#pragma unroll
        for (int j = 0; j < PS_ROWS; ++j) {
            if (j * PS_THREADS + tid >= item.qn) continue;
            const unsigned long long t = pair_term(best[j]);
            s_all += t;
            if (best[j] <= tau) { n_in += 1ull; s_in += t; }
        }
        n_in = wave_sum_u64(n_in); s_in = wave_sum_u64(s_in); s_all = wave_sum_u64(s_all);
        const unsigned long long nbad = wave_sum_u64((unsigned long long)bad);
        if (lane == 0) {
            atomicAdd(&s_sum[0], n_in); atomicAdd(&s_sum[1], s_in); atomicAdd(&s_sum[2], s_all); atomicAdd(&s_sum[3], nbad);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long* row = acc + (size_t)job.pair * PAIR_ACC_PITCH;
            atomicAdd(row + (job.q_src ? PAIR_N_SRC_IN : PAIR_N_TPL_IN), s_sum[0]);
            atomicAdd(row + (job.q_src ? PAIR_S_FWD_IN : PAIR_S_REV_IN), s_sum[1]);
            if (!job.q_src) atomicAdd(row + PAIR_S_REV_ALL, s_sum[2]);
            if (s_sum[3]) atomicAdd(row + PAIR_BAD, s_sum[3]);
        }
        __syncthreads();   // (s_sum and s_item are rewritten at the top)
    }
}

void launch_pair_score(hipStream_t s, int n_items, int n_wg, const PairJob* jobs, const PairItem* items, const float4* src, const float4* tpl, float tau,
                       unsigned long long* acc, int* queue) {
    if (n_items <= 0) return;
    hipLaunchKernelGGL(k_pair_score, dim3(std::max(1, std::min(n_items, n_wg))), dim3(PS_THREADS), 0, s, jobs, items, n_items, src, tpl, tau, acc, queue);
}

}  // namespace cd
