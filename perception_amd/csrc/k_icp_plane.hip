// k_icp_plane.hip - S6 with canonical rule C17 (perception_amd/icp_plane.py is the specification): the
// plane-weighted ICP step for LATTICE templates, opt-in through cd_set_icp_plane_weight.
//
// The ICP is k_icp_lat's - rule C5 correspondences by the closed-form lattice search (lat_search.hpp), rule C8's bound,
// X <- T X in place, Tfinal <- T Tfinal, DefaultConvergenceCriteria in icp_step's order (icp_step_tail), getFitnessScore over
// every point - with another transformation estimate: a weighted linear least-squares step in which the residual along the
// normal of the correspondence's face (a coordinate axis: IcpLattice::w) counts 1 and the two tangential components count
// lambda_it (1 until the MSE has once been <= switch_distance^2, tangent_weight from the next iteration on; a one-way latch).
// It is NOT pcl::registration::TransformationEstimationPointToPlaneLLS, which is the singular case lambda = 0.
//
// Shape: one workgroup of four waves keeps ONE (cluster, template) pair going for its whole ICP and then takes the next pair of
// the launch's queue (largest first), restaging the axis tables when the template changes.  Per iteration: the waves take the
// passes of 64 points - transform, search, the 27 terms + d2 of icp_plane_math.hpp as 28 rule-C4 integer sums in 56
// accumulator registers per lane (LatFix raw bits inside its range, fixq outside: the same integers), folded through DPP
// into LDS - barrier - lane 0 solves in double (plane_solve: 6 x 6 L D L^T, no square root, no library call) and runs the
// shared tail - barrier.  Integer sums: nothing depends on how points fall to lanes, waves or passes.
// 56 accumulators + the search do not fit the 128 registers of four waves per SIMD: the launch bounds ask for two
// (256 registers), which the compiler fills without scratch (has its report).
// No MFMA: nothing here is a dense contraction.  Results leave through ordinary vector stores.
#include "kernels.hpp"
#include "icp_solve.hpp"
#include "lat_search.hpp"
#include "icp_plane_math.hpp"

namespace cd {

constexpr int PLANE_WAVES = 4;
constexpr int PLANE_THREADS = PLANE_WAVES * WAVE;
constexpr int PLANE_D2 = PLANE_NSUMS - 1;   // plane_terms' d2: the one sum at FIX_SHIFT_D2
enum { PLANE_ITER = 0, PLANE_FIT = 1, PLANE_EMPTY = 2 };

struct PlaneItem {
    int k, src_off, n, tslot;   // the pair (problem index, first point, points, template slot)
    int phase;                  // PLANE_ITER / PLANE_FIT / PLANE_EMPTY
    int latched;                // rule C17 step 5
    int pad[2];
};

// BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter the sums; s_nv counts them
template <bool BOUNDED>
__global__ void __launch_bounds__(PLANE_THREADS, 2)
k_icp_plane(int nitems, const int* __restrict__ order, const IcpCluster* __restrict__ cl, IcpState* __restrict__ st,
            unsigned long long* __restrict__ accf, PlaneStats* __restrict__ pstat, const IcpLattice* __restrict__ lats,
            float4* __restrict__ src, const float4* __restrict__ src0, int* __restrict__ queue, IcpParams prm, IcpBound bnd, PlaneParams pp) {
    __shared__ float4 s_tab[LAT_MAX_TAB];
    __shared__ int4 s_face[2 * LAT_MAX_FACES];
    __shared__ unsigned long long s_acc[32];   // [0..27] the sums of the current step ([0]: the fitness sum in PLANE_FIT)
    __shared__ IcpState s_so;
    __shared__ PlaneItem s_it;
    __shared__ PlaneStats s_ps;
    __shared__ unsigned s_nv;
    const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
    if (threadIdx.x < 32) s_acc[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) s_nv = 0u;
    int cur_tslot = -1;
    for (;;) {
        // ---- the next live pair of the queue (lane 0) ----
        if (threadIdx.x == 0) {
            IcpCluster c;
            const int k = icp_pop_live(queue, nitems, order, cl, st, c);
            s_it.phase = k < 0 ? PLANE_EMPTY : PLANE_ITER;
            if (k >= 0) {
                s_it.k = k; s_it.src_off = c.src_off; s_it.n = c.n; s_it.tslot = c.slot;
                s_it.latched = pp.latched0;
                s_so = st[2 * (size_t)k];
                s_ps.plane_iterations = 0; s_ps.first_plane_iteration = 0; s_ps.stopped_singular = 0; s_ps.reserved = 0;
            }
        }
        __syncthreads();
        if (s_it.phase == PLANE_EMPTY) break;   // (uniform)
        const int n = __builtin_amdgcn_readfirstlane(s_it.n), src_off = __builtin_amdgcn_readfirstlane(s_it.src_off);
        const int tslot = __builtin_amdgcn_readfirstlane(s_it.tslot);
        const IcpLattice* __restrict__ L = lats + tslot;
        if (tslot != cur_tslot) {   // (uniform) another template: its tables and face words
            lat_stage_tables(L, L->ntab, s_tab, s_face, threadIdx.x, PLANE_THREADS);
            cur_tslot = tslot;
            __syncthreads();
        }
        LatFaces F;
        lat_faces_load(L, F);
        const int npass = (n + 63) >> 6;
        float4* pts = src + src_off;
        for (;;) {
            const int phase = __builtin_amdgcn_readfirstlane(s_it.phase);   // (settled behind the barrier that ended the last round)
            if (phase == PLANE_ITER) {
                const bool moved = s_so.iters > 0;   // X <- T*X from the second iteration on
                const float lam_it = s_it.latched ? pp.lambda : 1.0f;
                float T[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) T[i] = s_so.T[i];
                unsigned long long SA[16], SB[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) { SA[i] = 0ull; SB[i] = 0ull; }   // (SB[12..15] stay zero and are never folded)
                unsigned nv = 0u;
                lat_for_passes<PLANE_WAVES>(pts, n, sub, lane, [&](int myq, bool act, const float4& p) {
                    float px = p.x, py = p.y, pz = p.z;
                    if (moved) {   // written back by the lane that owns the point
                        xform(T, p.x, p.y, p.z, px, py, pz);
                        if (act) pts[myq] = make_float4(px, py, pz, p.w);
                    }
                    const LatHit h = lat_nearest_any<true, true>(s_tab, s_face, F, px, py, pz);
                    const int w = s_face[min(max(h.face, 0), LAT_MAX_FACES - 1)].x;   // the face's constant axis = its normal
                    const bool keep = act && (!BOUNDED || h.d <= bnd.d2_max);
                    if constexpr (BOUNDED) nv += (unsigned)__popcll(ballot64(keep));
                    if (keep) {
                        const float pv[3] = {px, py, pz}, qv[3] = {h.nx, h.ny, h.nz};
                        float t[PLANE_NSUMS];
                        plane_terms(pv, qv, w, lam_it, h.d, t);
                        // LatFix's range: every term below 2^18 (coordinates below 256 m, a neighbour less than 128 m away, weights
                        // <= 1); outside it the general conversion - the same integers either way (a NaN fails the test)
                        const float big_c = fmaxf(fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)), fmaxf(fmaxf(fabsf(h.nx), fabsf(h.ny)), fabsf(h.nz)));
                        unsigned long long b[PLANE_NSUMS];
                        lat_fix_terms<PLANE_D2>(t, big_c < 256.f && h.d < 16384.f, b);
#pragma unroll
                        for (int i = 0; i < PLANE_NSUMS; ++i) (i < 16 ? SA[i] : SB[i - 16]) += b[i];
                    }
                });
                if (sub < npass) {
                    wave_fold_to_lds(SA, 16, s_acc);
                    wave_fold_to_lds(SB, 12, s_acc + 16);
                }
                if constexpr (BOUNDED) { if (sub < npass && lane == 0) atomicAdd(&s_nv, nv); }
            } else {
                // (T is the identity after a stop)
                lat_fitness_pass<PLANE_WAVES>(pts, src0 + src_off, n, sub, lane, s_so, s_tab, s_face, F, s_acc);
            }
            __syncthreads();
            // ---- lane 0: the step (estimate, latch, shared tail), or the pair's results ----
            if (threadIdx.x == 0) {
                if (phase == PLANE_ITER) {
                    // (every kept point added the constant of its scale to each sum: LatFix)
                    const int nv = BOUNDED ? (int)s_nv : n;
                    int done;
                    if (nv < ICP_MIN_CORR) {
                        icp_stop_few(s_so);
                        done = 1;
                    } else {
                        long long A[PLANE_NSUMS];
#pragma unroll
                        for (int i = 0; i < PLANE_NSUMS; ++i)
                            A[i] = (long long)(s_acc[i] - lat_fix_offset(i == PLANE_D2, (unsigned long long)nv));
                        float Tn[16];
                        if (plane_solve(A, nv, Tn)) {   // singular: stops before the update, as too few correspondences do
                            icp_stop_few(s_so);
                            s_ps.stopped_singular = 1;
                            done = 1;
                        } else {
                            const double mse = unfix((unsigned long long)A[27], FIX_SHIFT_D2) / (double)nv;
                            if (s_it.latched) {
                                s_ps.plane_iterations += 1;
                                if (s_ps.first_plane_iteration == 0) s_ps.first_plane_iteration = s_so.iters + 1;
                            }
                            if (mse <= pp.switch2) s_it.latched = 1;
                            done = icp_step_tail(s_so, Tn, (unsigned long long)A[27], nv, prm);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < PLANE_NSUMS; ++i) s_acc[i] = 0ull;
                    if constexpr (BOUNDED) s_nv = 0u;
                    if (done) s_it.phase = PLANE_FIT;
                } else {
                    const int k = s_it.k;
                    s_so.done = 1;
                    st[2 * (size_t)k] = s_so;
                    st[2 * (size_t)k + 1] = s_so;
                    accf[k] = s_acc[0] - lat_fix_offset(true, (unsigned long long)n);
                    pstat[k] = s_ps;
                    s_acc[0] = 0ull;
                }
            }
            __syncthreads();
            if (phase == PLANE_FIT) break;   // (uniform) the pair is finished: the next one
        }
    }
}

void launch_icp_plane(hipStream_t s, int nitems, int n_wg, const IcpProblems& P, PlaneStats* pstat, const IcpTemplates& T, const IcpScratch& S,
                      IcpParams prm, const IcpBound& bnd, const PlaneParams& pp) {
    if (nitems <= 0 || n_wg <= 0) return;
    if (bnd.bounded)
        hipLaunchKernelGGL((k_icp_plane<true>), dim3(n_wg), dim3(PLANE_THREADS), 0, s, nitems, P.order, P.cl, P.st, P.accf, pstat, T.lats, S.src, S.src0, S.queue, prm, bnd, pp);
    else
        hipLaunchKernelGGL((k_icp_plane<false>), dim3(n_wg), dim3(PLANE_THREADS), 0, s, nitems, P.order, P.cl, P.st, P.accf, pstat, T.lats, S.src, S.src0, S.queue, prm, bnd, pp);
}

}  // namespace cd
