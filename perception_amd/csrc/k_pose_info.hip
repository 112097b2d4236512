// k_pose_info.hip - canonical rule C23 (perception_amd/pose_info.py is the specification): the pose information of
// (cluster, lattice template) results, opt-in through cd_set_pose_info, and the kernel behind cd_pose_info_points.
//
// What it reports: which of the six directions of a small rigid motion a result's correspondences constrain and by how many
// points' worth, the covariance of the pose over the constrained ones and the twist the data says least about.  It counts what
// the template's SURFACES constrain and nothing else: the outline of a partial view adds nothing, and hidden faces are not
// reasoned about.
//
// Shape (k_icp_plane's, without the iteration): one workgroup of four waves takes (cluster, slot) items from the launch's queue -
// the host has sorted them largest first - staging the slot's axis tables and face words in LDS only when the slot changes.  ONE
// pass over the cluster's points, 64 per wave at a time: the point under T (xform_row, rule C21's step 1), its neighbour and the
// face by the closed-form lattice search (lat_search.hpp: lat_nearest_axes for one face per axis, lat_nearest otherwise), rule
// C8's bound, the six terms of pose_info_math.hpp.  A point adds to the six sums of ITS face's axis only, so the lane keeps three
// banks of six 64-bit accumulators (36 registers) and each bank is added to under its own mask - no 18 always-added sums of
// mostly zero terms.  Terms inside LatFix's range enter as raw bits (three instructions), the others through fixq: the same
// integers, and the counts of the banks tell the last lane how many constants to take off.  The banks fold through DPP into LDS
// (wave_fold_to_lds); after a barrier lane 0 runs pose_finish in double - the matrices of its Jacobi live in LDS, indexed at run
// time - and writes the record with ordinary vector stores.  Integer sums and counts: nothing depends on how points fall to
// lanes, waves, passes or workgroups.  No MFMA: nothing here is a dense contraction.
// Budget (compiler's report, gfx950): DESIGN.md §2, C23.
#include "kernels.hpp"
#include "lat_search.hpp"
#include "pose_info_math.hpp"

namespace cd {

constexpr int POSE_WAVES = 4;
constexpr int POSE_THREADS = POSE_WAVES * WAVE;
static_assert(POSE_AXIS_SUMS == 6 && POSE_NSUMS <= 32, "three banks of six sums, folded as one array of 16 and one of 2");

__global__ void __launch_bounds__(POSE_THREADS, 2)
k_pose_info(int nitems, const PoseItem* __restrict__ items, const IcpLattice* __restrict__ lats, const float4* __restrict__ src0, float tau,
            double min_support, cd_pose_info* __restrict__ out, int* __restrict__ queue) {
    __shared__ float4 s_tab[LAT_MAX_TAB];
    __shared__ int4 s_face[2 * LAT_MAX_FACES];
    __shared__ unsigned long long s_acc[32];   // [6 a + j]: sum j of axis a
    __shared__ unsigned s_cnt[4];              // kept points per axis, points with a non-finite coordinate
    __shared__ double s_ws[POSE_WS];
    __shared__ int s_item;
    const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
    int cur_slot = -1;
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(queue, 1);
        if (threadIdx.x < 32) s_acc[threadIdx.x] = 0ull;
        if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
        __syncthreads();
        const int it = __builtin_amdgcn_readfirstlane(s_item);
        if (it >= nitems) return;   // (the whole workgroup)
        const PoseItem* __restrict__ I = items + it;
        const int n = __builtin_amdgcn_readfirstlane(I->n), src_off = __builtin_amdgcn_readfirstlane(I->src_off);
        const int slot = __builtin_amdgcn_readfirstlane(I->slot);
        const IcpLattice* __restrict__ L = lats + slot;
        if (slot != cur_slot) {   // (uniform) another template: its tables and face words
            lat_stage_tables(L, L->ntab, s_tab, s_face, threadIdx.x, POSE_THREADS);
            cur_slot = slot;
            __syncthreads();
        }
        LatFaces F;
        lat_faces_load(L, F);
        float T[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = I->T[i];
        const float cx = I->c0[0], cy = I->c0[1], cz = I->c0[2];
        const float4* __restrict__ pts = src0 + src_off;
        const int npass = (n + 63) >> 6;
        unsigned long long SA[16], SB[16];   // sums 0 .. 15 and 16, 17 (SB[2..15] stay zero and are never folded)
#pragma unroll
        for (int i = 0; i < 16; ++i) { SA[i] = 0ull; SB[i] = 0ull; }
        unsigned c0n = 0u, c1n = 0u, c2n = 0u, nbad = 0u;
        lat_for_passes<POSE_WAVES>(pts, n, sub, lane, [&](int, bool act, const float4& p) {
            const float ax = xform_row(T, 0, p.x, p.y, p.z), ay = xform_row(T, 1, p.x, p.y, p.z), az = xform_row(T, 2, p.x, p.y, p.z);
            const bool fin = pose_finite(ax, ay, az);
            nbad += (unsigned)__popcll(ballot64(act && !fin));
            const LatHit h = lat_nearest_any<true, true>(s_tab, s_face, F, ax, ay, az);
            const int4 fd = s_face[min(max(h.face, 0), LAT_MAX_FACES - 1)];
            const int w = fd.x;   // the face's constant axis = its normal; fd.w: its constant coordinate = the neighbour's on that axis
            const bool keep = act && fin && h.d <= tau;
            const uint64_t k0 = ballot64(keep && w == 0), k1 = ballot64(keep && w == 1), k2 = ballot64(keep && w == 2);
            c0n += (unsigned)__popcll(k0); c1n += (unsigned)__popcll(k1); c2n += (unsigned)__popcll(k2);
            if (k0 | k1 | k2) {   // (uniform)
                float t[POSE_AXIS_SUMS];
                pose_terms(ax, ay, az, cx, cy, cz, w, __int_as_float(fd.w), t);
                unsigned long long b[POSE_AXIS_SUMS];
                // LatFix's range: |p| < 512 makes every term at 2^32 smaller than 2^18, r r < 2^14 at 2^36 (a NaN fails the test)
                lat_fix_terms<POSE_RR>(t, fabsf(t[0]) < POSE_FIX_P_MAX && fabsf(t[1]) < POSE_FIX_P_MAX && t[5] < POSE_FIX_R_MAX * POSE_FIX_R_MAX, b);
                if (keep && w == 0) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) SA[j] += b[j];
                }
                if (keep && w == 1) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) SA[6 + j] += b[j];
                }
                if (keep && w == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) SA[12 + j] += b[j];
                    SB[0] += b[4]; SB[1] += b[5];
                }
            }
        });
        if (sub < npass) {
            wave_fold_to_lds(SA, 16, s_acc);
            wave_fold_to_lds(SB, 2, s_acc + 16);
            if (lane == 0) {
                atomicAdd(&s_cnt[0], c0n); atomicAdd(&s_cnt[1], c1n); atomicAdd(&s_cnt[2], c2n);
                if (nbad) atomicAdd(&s_cnt[3], nbad);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // (every kept point added the constant of its scale to each sum of its bank: LatFix)
#pragma unroll 1
            for (int i = 0; i < POSE_NSUMS; ++i)
                s_acc[i] -= lat_fix_offset(i % POSE_AXIS_SUMS == POSE_RR, s_cnt[i / POSE_AXIS_SUMS]);
            pose_finish(n, (int)s_cnt[3], (int)s_cnt[0], (int)s_cnt[1], (int)s_cnt[2], reinterpret_cast<const long long*>(s_acc), cx, cy, cz, I->length,
                        min_support, I->accepted, s_ws, out + I->pair);
        }
        __syncthreads();   // (s_item, s_acc and s_cnt are rewritten at the top)
    }
}

void launch_pose_info(hipStream_t s, int nitems, int n_wg, const PoseItem* items, const IcpLattice* lats, const float4* src0, float tau, double min_support,
                      cd_pose_info* out, int* queue) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_pose_info, dim3(std::max(1, std::min(nitems, n_wg))), dim3(POSE_THREADS), 0, s, nitems, items, lats, src0, tau, min_support, out, queue);
}

}  // namespace cd
