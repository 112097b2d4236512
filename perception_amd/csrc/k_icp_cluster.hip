// k_icp_cluster.hip - S6 ICP, whole-cluster driver: one workgroup runs a cluster's complete ICP, a workgroup barrier per iteration.
#include "kernels.hpp"
#include "icp_solve.hpp"
#include "icp_search.hpp"

namespace cd {

// ---------------------------------------------------------------------------------------
// Whole-cluster variant (batch mode): ONE persistent workgroup takes a cluster from the queue
// (largest first) and runs its complete ICP - every iteration's transform, search, moments,
// Umeyama/SVD solve and convergence test, then the fitness pass - without leaving the CU.
// Same arithmetic as k_icp_solve + k_icp_iter + k_icp_fitness (the moments are order-free
// integer sums), so the results are bit-identical; what disappears are the ~2 launches per
// iteration, the global moment atomics, the host completion polls and the under-filled tail.
// ---------------------------------------------------------------------------------------
// The search of one pass of k_icp_cluster, in two steps.  First the near queries - seed
// ball at most rmax wide, none unless the resident template has a cell table (grid_ok) -, a lane each, by the walk of the grid
// cells the ball touches; returns whether this lane's query was one.
__device__ __forceinline__ bool search_near(const float4* s_tpl, const unsigned short* s_cs, const IcpGrid& g, bool grid_ok, float rmax,
                                            int gpad, QueryRegs& q, int nk) {
    float rr = 0.f;
    bool near = false;
    if ((int)(threadIdx.x & 63) < nk && grid_ok) { rr = __fmul_rn(__fsqrt_rn(q.pbest), 1.0f + 2.0e-6f); near = rr <= rmax; }
    if (ballot64(near)) grid_search(s_tpl, s_cs, g, near, rr, q, gpad);
    return near;
}
// Then the rest, a wave per query, over the run boxes of the resident image; a template of more than ICPT_TPL_LDS points has no
// near queries and is searched ICPT_TPL_LDS points at a time.
__device__ __forceinline__ void search_rest(const TplRef& t, int m, bool near, QueryRegs& q, int nk, float4* s_tpl, RunBoxes& bx,
                                            int& staged) {
    const int lane = threadIdx.x & 63;
    if (m <= ICPT_TPL_LDS) {
        search_chunk(s_tpl, bx, 0, m, q, ballot64(lane < nk && !near));
    } else {
        search_fixed_chunks(t, m, q, nk, s_tpl, bx);
        staged = -1;
    }
}

__device__ __forceinline__ void block_sum16(unsigned long long (&S)[16], unsigned long long (*s_part)[16],
                                            unsigned long long* s_tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const unsigned long long t = wave_sum_u64(S[k]);
        if (lane == 0) s_part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        unsigned long long t = 0ull;
#pragma unroll
        for (int w = 0; w < ICPT_WAVES; ++w) t += s_part[w][threadIdx.x];
        s_tot[threadIdx.x] = t;
    }
    __syncthreads();
}

// BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter the sums; s_nv counts them (one LDS add per wave)
template <bool BOUNDED>
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_cluster(int ncl, const int* __restrict__ order,
                                                              const IcpCluster* __restrict__ cl, IcpState* __restrict__ st,
                                                              unsigned long long* __restrict__ accf,
                                                              const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                              const float4* __restrict__ thi,
                                                              const IcpGrid* __restrict__ grids,
                                                              const unsigned short* __restrict__ tcell, float4* src,
                                                              const float4* __restrict__ src0, int* nn, int* queue,
                                                              IcpParams prm, IcpBound bnd) {
    __shared__ float4 s_tpl[ICPT_IMG];
    __shared__ unsigned short s_cs[ICP_MAX_CELLS + 8];   // cell start table of the staged template
    __shared__ unsigned long long s_part[ICPT_WAVES][16];
    __shared__ unsigned long long s_tot[16];
    __shared__ IcpState s_so;   // the cluster's ICP state (T = current transformation_, Tfinal = accumulated)
    __shared__ int s_flag[2];   // [0] queue item, [1] done
    __shared__ uint32_t s_nv;   // (BOUNDED) kept correspondences of the current iteration
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RunBoxes bx;
    int staged = -1;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_flag[0] = atomicAdd(queue, 1);
        if (BOUNDED && threadIdx.x == 0) s_nv = 0u;
        __syncthreads();
        const int item = s_flag[0];
        if (item >= ncl) break;
        const int k = order[item];
        const IcpCluster c = cl[k];
        if (st[2 * (size_t)k].done) continue;            // host pre-marked (too few points / no template)
        const TplRef tr = tpl_ref(tpl, tlo, thi, c.tpl_off);
        const float4* tp = tr.p;
        const bool resident = c.tpl_m <= ICPT_TPL_LDS;
        const IcpGrid g = grids[c.slot];
        const bool grid_ok = resident && g.ncell > 0;
        const float rmax = __fmul_rn(prm.grid_rc, g.cell);
        const int gpad = (c.tpl_m + ICP_SUB - 1) / ICP_SUB * ICP_SUB;   // first point of the +inf pad run of the staged image
        if (resident && staged != c.tpl_off) {
            __syncthreads();
            if (grid_ok) for (int i = threadIdx.x; i <= g.ncell; i += ICPT_THREADS) s_cs[i] = tcell[g.cell_off + i];
            stage_chunk(tp, tr.lo, tr.hi, 0, c.tpl_m, s_tpl, bx);
            staged = c.tpl_off;
        }
        float4* pts = src + c.src_off;
        const float4* pts0 = src0 + c.src_off;
        int* nnq = nn + c.src_off;
        if (threadIdx.x == 0) s_so = st[2 * (size_t)k];   // thread 0 owns and updates it
        int it = 0;
        for (;; ++it) {
            unsigned long long S[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) S[i] = 0ull;
            uint32_t nv = 0u;   // (BOUNDED: this wave's kept correspondences, wave-uniform)
            for (int q0 = 0; q0 < c.n; q0 += ICPT_THREADS) {
                const int nq = min(ICPT_THREADS, c.n - q0);
                const int myq = q0 + wave * WAVE + lane;   // a wave takes 64 consecutive points: coalesced, and neighbours in
                QueryRegs q;                               // voxel order have neighbouring answers (less divergence per pass)
                int nk;
                // fetch (+ X <- T*X written back by the lane that owns the point)
                nk = min(WAVE, max(0, nq - wave * WAVE));
                q.px = q.py = q.pz = q.pbest = 0.f; q.pbi = 0; q.poi = 0x7fffffff;
                if (lane < nk) {
                    const float4 p = pts[myq];
                    q.px = p.x; q.py = p.y; q.pz = p.z;
                    if (it > 0) {
                        xform(s_so.T, p.x, p.y, p.z, q.px, q.py, q.pz);   // T read from LDS to keep registers free
                        pts[myq] = make_float4(q.px, q.py, q.pz, p.w);
                    }
                    // seed_query(tp, c.tpl_m, it > 0, it < 3, &nnq[myq], q) written out: called here it costs every pass a branch (profiles/EXPERIMENTS.md)
                    q.pbest = 3.402823466e38f;
                    if (it > 0) {
                        q.pbi = nnq[myq];
                        const float4 q0p = tp[q.pbi];
                        q.pbest = dist2(q.px, q.py, q.pz, q0p.x, q0p.y, q0p.z);
                    }
                    if (it < 3) {
                        for (int j = 0; j < c.tpl_m; j += ICP_SUB) {
                            const float4 t = tp[j];
                            const float d = dist2(q.px, q.py, q.pz, t.x, t.y, t.z);
                            if (d < q.pbest) { q.pbest = d; q.pbi = j; }
                        }
                    }
                    q.pbest = seed_bound(q.pbest);
                    q.poi = __float_as_int(tp[q.pbi].w);
                }
                const bool near = search_near(s_tpl, s_cs, g, grid_ok, rmax, gpad, q, nk);
                search_rest(tr, c.tpl_m, near, q, nk, s_tpl, bx, staged);
                if constexpr (BOUNDED) nv += (uint32_t)__popcll(ballot64(lane < nk && q.pbest <= bnd.d2_max));
                if (lane < nk) {
                    nnq[myq] = q.pbi;
                    if (!BOUNDED || q.pbest <= bnd.d2_max) {
                        const float4 qq = resident ? s_tpl[q.pbi] : tp[q.pbi];
                        const float pv[3] = {q.px, q.py, q.pz}, qv[3] = {qq.x, qq.y, qq.z};
                        unsigned long long t[16];
                        moment_terms(pv, qv, q.pbest, t);
#pragma unroll
                        for (int i = 0; i < 16; ++i) S[i] += t[i];
                    }
                }
            }
            if constexpr (BOUNDED) { if (lane == 0 && nv) atomicAdd(&s_nv, nv); }
            block_sum16(S, s_part, s_tot);
            const int n_used = BOUNDED ? (int)s_nv : c.n;
            if (threadIdx.x == 0) {   // the state update for iteration it+1
                s_flag[1] = icp_step<BOUNDED>(s_so, s_tot, n_used, prm);
                if (BOUNDED) s_nv = 0u;
            }
            __syncthreads();
            if (s_flag[1]) break;
        }
        // final X <- T*X (PCL transforms before it tests convergence), then getFitnessScore()
        {
            unsigned long long S[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) S[i] = 0ull;
            for (int q0 = 0; q0 < c.n; q0 += ICPT_THREADS) {
                const int nq = min(ICPT_THREADS, c.n - q0);
                const int myq = q0 + wave * WAVE + lane;
                const int nk = min(WAVE, max(0, nq - wave * WAVE));
                QueryRegs q;
                q.px = q.py = q.pz = q.pbest = 0.f; q.pbi = 0; q.poi = 0x7fffffff;
                if (lane < nk) {
                    const float4 p = pts[myq];
                    float ox, oy, oz;
                    xform(s_so.T, p.x, p.y, p.z, ox, oy, oz);
                    pts[myq] = make_float4(ox, oy, oz, p.w);
                    const float4 p0 = pts0[myq];
                    xform(s_so.Tfinal, p0.x, p0.y, p0.z, q.px, q.py, q.pz);
                    seed_query(tp, c.tpl_m, true, false, &nnq[myq], q);
                }
                const bool near = search_near(s_tpl, s_cs, g, grid_ok, rmax, gpad, q, nk);
                search_rest(tr, c.tpl_m, near, q, nk, s_tpl, bx, staged);
                if (lane < nk) S[0] += (unsigned long long)fixq(q.pbest, FIX_SHIFT_D2);
            }
            block_sum16(S, s_part, s_tot);
            if (threadIdx.x == 0) {
                s_so.done = 1;
                st[2 * (size_t)k] = s_so;
                st[2 * (size_t)k + 1] = s_so;
                accf[k] = s_tot[0];
            }
        }
    }
}

void launch_icp_cluster(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_cu, IcpParams prm, const IcpBound& bnd) {
    if (ncl <= 0) return;
    hipLaunchKernelGGL(bnd.bounded ? k_icp_cluster<true> : k_icp_cluster<false>, dim3(ncl < n_cu ? ncl : n_cu), dim3(ICPT_THREADS), 0, s, ncl, P.order, P.cl, P.st, P.accf,
                       T.tpl, T.tlo, T.thi, T.grids, T.tcell, S.src, S.src0, S.nn, S.queue, prm, bnd);
}

}  // namespace cd
