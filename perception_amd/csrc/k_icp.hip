// k_icp.hip - S6 point-to-point ICP of every cluster against a template.
//
// Replaces pcl::IterativeClosestPoint<PointXYZ,PointXYZ>::align + getFitnessScore (reference:
// cuboid_detection/src/iterative_closest_point.cpp:170-182,
// object_detection/src/object_pose_detection.cpp:220-235; maxIter 5000, transformation
// epsilon 1e-9, euclidean fitness epsilon = icp_fitness_score, no rejectors).  The reference leaves
// setMaxCorrespondenceDistance commented out; cd_set_icp_max_correspondence_distance provides it (rule C8,
// DESIGN.md): every kernel below has a BOUNDED instantiation that keeps a correspondence iff its d2 <= d2_max,
// after the same exact, unbounded search, and counts the kept ones for the solve.
//
// One launch == one PCL iteration for ALL clusters of ALL frames in the batch:
//   prologue (one lane per block, redundantly - it is ~2 us of scalar work and removes every
//             inter-workgroup hand-off): TransformationEstimationSVD (pcl::umeyama, Eigen
//             JacobiSVD restated in float32) from the 16 fixed-point moments the previous
//             launch accumulated, T_final <- T*T_final, DefaultConvergenceCriteria;
//   body    : X <- T*X (in place), exact brute-force nearest neighbour of every source point
//             over the template staged through LDS in 2048-point (32 KiB) chunks - every lane
//             reads the same LDS address (broadcast), ties keep the lowest template index -,
//             then the 16 moments {sum p, sum q, sum q p^T, sum d2} as 64-bit fixed point:
//             wave butterfly + one atomic per wave (order-free, hence bit-reproducible).
// State is double-buffered by launch parity and the moment buffers rotate mod 3, so no block
// ever reads a word another block writes in the same launch.
// No MFMA: the only matrix objects are 3x3; the pair loop is 8 dependent f32 VALU ops.
//
// This unit holds the sliced multi-launch kernels and their persistent form (k_icp_persist); the whole-cluster drivers are
// k_icp_cluster.hip and k_icp_pipe.hip, the searches all three share icp_search.hpp.
#include "kernels.hpp"
#include "icp_solve.hpp"
#include "icp_debug.hpp"
#include "icp_search.hpp"

namespace cd {

// Templates that do not fit LDS are searched chunk by chunk.  With a chunk table (IcpGrid: whole k-d subtrees, i.e. compact
// regions, with their boxes) a workgroup stages a chunk only when its box comes within the running bound of SOME query of
// the workgroup - once the cloud sits on the template a slice of neighbouring queries needs one or two chunks, not all.
// Exact for the same reason as the run boxes: the chunk box's lower bound is below that of every run box inside it, so a
// skipped chunk holds only runs that the search would have pruned.  Returns the wave's queries (lane mask) that need the
// chunk; *any_in_wg says whether the workgroup needs it at all.  Contains two barriers: call from all threads.
__device__ __forceinline__ unsigned long long chunk_needed(const IcpGrid& g, int ci, const QueryRegs& q, int nk, int* s_flag,
                                                           bool* any_in_wg) {
    const int lane = threadIdx.x & 63;
    const float4 L = make_float4(g.chunk_lo[ci][0], g.chunk_lo[ci][1], g.chunk_lo[ci][2], 0.f);
    const float4 H = make_float4(g.chunk_hi[ci][0], g.chunk_hi[ci][1], g.chunk_hi[ci][2], 0.f);
    const unsigned long long m = ballot64(lane < nk && box_lb(L, H, q.px, q.py, q.pz) <= q.pbest);
    if (threadIdx.x == 0) *s_flag = 0;
    __syncthreads();
    if (lane == 0 && m) atomicOr(s_flag, 1);
    __syncthreads();
    *any_in_wg = *s_flag != 0;
    return m;
}

// Batched fetch of the wave's queries + seeds (one round of global loads per wave).
// use_prev: seeds are the previous launch's neighbours (nn[]); coarse: also try the first point of
// every run (worth its m/64 tests while the cloud still moves a lot between launches).
__device__ __forceinline__ void fetch_queries(const float4* __restrict__ tpl, int m, const float4* pts, int nq, bool use_prev,
                                              bool coarse, bool apply_T, const float* Tm, const int* nn, QueryRegs& q, int& nk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int myq = wave + ICPT_WAVES * lane;
    nk = nq > wave ? (nq - wave + ICPT_WAVES - 1) / ICPT_WAVES : 0;
    q.px = q.py = q.pz = q.pbest = 0.f;
    q.pbi = 0; q.poi = 0x7fffffff;
    if (lane < nk) {
        const float4 p = pts[myq];
        q.px = p.x; q.py = p.y; q.pz = p.z;
        if (apply_T) xform(Tm, p.x, p.y, p.z, q.px, q.py, q.pz);
        seed_query(tpl, m, use_prev, coarse || !use_prev, &nn[myq], q);
    }
}

__device__ __forceinline__ void store_queries(const QueryRegs& q, int nk, int* nn, float* d2buf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < nk) {
        nn[wave + ICPT_WAVES * lane] = q.pbi;
        d2buf[wave + ICPT_WAVES * lane] = q.pbest;
    }
}

// ---------------------------------------------------------------------------------------
// What the sliced drivers do with one slice of queries - search, moments, fitness - is written once, here: k_icp_iter,
// k_icp_persist and k_icp_fitness compute the same thing by construction (the chunk walk they share with k_icp_cluster is
// icp_search.hpp's).  All of these contain barriers: call them from all threads.
// ---------------------------------------------------------------------------------------
// Search the wave's queries against cluster c's template.  `staged` is the template offset whose whole image (and this
// lane's boxes in bx) is resident in s_tpl, -1 for none: a template that fits LDS is staged only when another one is
// resident, and any chunked walk leaves -1 behind, so that the next small template is staged again.
__device__ __forceinline__ void search_slice(const TplRef& t, const IcpCluster& c, const IcpGrid* __restrict__ grids, QueryRegs& q,
                                             int nk, float4* s_tpl, RunBoxes& bx, int& staged, int* s_flag) {
    if (c.tpl_m <= ICPT_TPL_LDS) {
        if (staged != c.tpl_off) { stage_chunk(t.p, t.lo, t.hi, 0, c.tpl_m, s_tpl, bx); staged = c.tpl_off; }
        search_chunk(s_tpl, bx, 0, c.tpl_m, q, lanes_below(nk));
        return;
    }
    const IcpGrid& g = grids[c.slot];
    if (g.nchunk > 0) {
        for (int ci = 0; ci < g.nchunk; ++ci) {
            bool any;
            const unsigned long long todo = chunk_needed(g, ci, q, nk, s_flag, &any);
            if (!any) continue;
            stage_chunk(t.p, t.lo, t.hi, g.chunk_start[ci], g.chunk_n[ci], s_tpl, bx);
            search_chunk(s_tpl, bx, g.chunk_start[ci], g.chunk_n[ci], q, todo);
        }
    } else {
        search_fixed_chunks(t, c.tpl_m, q, nk, s_tpl, bx);
    }
    staged = -1;
}

// X <- T * X of one slice, in place (T: 12 floats, row-major)
__device__ __forceinline__ void transform_slice(const float* Tm, float4* pts, int nq) {
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tm[k];
    for (int i = threadIdx.x; i < nq; i += ICPT_THREADS) {
        const float4 p = pts[i];
        float ox, oy, oz;
        xform(T, p.x, p.y, p.z, ox, oy, oz);
        pts[i] = make_float4(ox, oy, oz, p.w);
    }
}

// The 16 fixed-point moments of a slice's correspondences (nnq, d2q: what store_queries wrote, behind a barrier), added to
// acc[slot] with slot = cluster * 3 + it % 3: per-point terms go to LDS (term-major, conflict-free), 8 terms at a time; wave
// k then sums term k.  BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter; bnd.ncorr[slot] counts them.
// s_scr (8 * ICP_QSLICE words) is still being read when this returns.
template <bool BOUNDED>
__device__ __forceinline__ void slice_moments(const float4* pts, const float4* __restrict__ tp, const int* nnq, const float* d2q, int nq,
                                              unsigned long long* acc, const IcpBound& bnd, size_t slot, unsigned long long* s_scr) {
    static_assert(ICP_QSLICE <= ICPT_THREADS, "one point per thread in the moment pass");
    const int lane = threadIdx.x & 63;
    unsigned long long S[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) S[k] = 0ull;
    const bool keep = threadIdx.x < nq && (!BOUNDED || icp_in_k0(d2q[threadIdx.x], bnd.d2_max));
    if constexpr (BOUNDED) {
        const unsigned long long kb = ballot64(keep);
        if (lane == 0 && kb) atomicAdd(&bnd.ncorr[slot], (uint32_t)__popcll(kb));
    }
    if (keep) {
        const int i = threadIdx.x;
        const float4 p = pts[i];
        const float4 qq = tp[nnq[i]];
        const float pv[3] = {p.x, p.y, p.z}, qv[3] = {qq.x, qq.y, qq.z};
        moment_terms(pv, qv, d2q[i], S);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();
        if (threadIdx.x < ICP_QSLICE) {
#pragma unroll
            for (int k = 0; k < 8; ++k) s_scr[k * ICP_QSLICE + threadIdx.x] = S[8 * h + k];
        }
        __syncthreads();
        const int k = threadIdx.x >> 6;   // waves 0..7 <-> the 8 moments of this half
        if (k < 8) {
            unsigned long long t = 0ull;
#pragma unroll
            for (int j = 0; j < ICP_QSLICE / 64; ++j) t += s_scr[k * ICP_QSLICE + j * 64 + lane];
            t = wave_sum_u64(t);
            if (lane == 0) atomicAdd(&acc[slot * 16 + 8 * h + k], t);
        }
    }
}

// getFitnessScore() of one slice: the neighbours of Tfinal * (original points), left in nnq / d2q; returns this thread's
// share of the slice's fixed-point sum of squared distances.
__device__ __forceinline__ unsigned long long slice_fitness(const TplRef& t, const IcpCluster& c, const IcpGrid* __restrict__ grids,
                                                            const float* Tfinal, const float4* pts0, int nq, int* nnq, float* d2q,
                                                            float4* s_tpl, RunBoxes& bx, int& staged, int* s_flag) {
    QueryRegs q;
    int nk;
    fetch_queries(t.p, c.tpl_m, pts0, nq, true, false, true, Tfinal, nnq, q, nk);
    search_slice(t, c, grids, q, nk, s_tpl, bx, staged, s_flag);
    store_queries(q, nk, nnq, d2q);
    __syncthreads();
    unsigned long long v = 0ull;
    for (int i = threadIdx.x; i < nq; i += ICPT_THREADS) v += (unsigned long long)fixq(d2q[i], FIX_SHIFT_D2);
    return v;
}

// One thread per cluster: the state update of launch `it` (icp_step: TransformationEstimationSVD + final_transformation_
// update + DefaultConvergenceCriteria), from the moments launch it-1 accumulated.
// Writes the state slot k_icp_iter(it) consumes, keeps the `done` flag in both parity slots and
// clears the moment buffer launch it+1 will accumulate into.  BOUNDED (rule C8): n = the kept correspondences that launch
// it-1 counted in bnd.ncorr; fewer than three stop the ICP before the update (icp_stop_few).
template <bool BOUNDED>
__global__ void __launch_bounds__(WAVE) k_icp_solve(int it, int ncl, const IcpCluster* __restrict__ cl,
                                                    IcpState* __restrict__ st, unsigned long long* __restrict__ acc,
                                                    int* __restrict__ queue, IcpParams prm, IcpBound bnd) {
    const int k = blockIdx.x * WAVE + threadIdx.x;
    if (k == 0) *queue = 0;   // work queue of the k_icp_iter launch that follows
    if (k >= ncl) return;
    const IcpState* sin = st + (size_t)k * 2 + (it & 1);
    IcpState* sout = st + (size_t)k * 2 + ((it + 1) & 1);
    *sout = *sin;
    if (sin->done) return;
    if (it > 0) {
        const unsigned long long* A = acc + ((size_t)k * 3 + (it - 1) % 3) * 16;
        const int n = BOUNDED ? (int)bnd.ncorr[(size_t)k * 3 + (it - 1) % 3] : cl[k].n;
        sout->done = icp_step<BOUNDED>(*sout, A, n, prm);
    }
    unsigned long long* Z = acc + ((size_t)k * 3 + (it + 1) % 3) * 16;
    for (int i = 0; i < 16; ++i) Z[i] = 0ull;
    if (BOUNDED) bnd.ncorr[(size_t)k * 3 + (it + 1) % 3] = 0u;
}

// Persistent: one workgroup per CU.  The template image and this lane's run boxes stay resident
// while the workgroup pulls (cluster, slice) work items from an atomic queue (zeroed by k_icp_solve).
// BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter the sums; bnd.ncorr[cluster][it % 3] counts them.
template <bool BOUNDED>
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_iter(int it, int n_work, const IcpWork* __restrict__ work,
                                                           const IcpCluster* __restrict__ cl, const IcpState* __restrict__ st,
                                                           unsigned long long* __restrict__ acc,
                                                           const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                           const float4* __restrict__ thi, const IcpGrid* __restrict__ grids,
                                                           float4* src, int* nn, float* d2buf, int qslice, int* queue,
                                                           IcpBound bnd) {
    __shared__ float4 s_tpl[ICPT_IMG];
    __shared__ unsigned long long s_scr[8 * ICP_QSLICE];   // moment scratch, 8 terms at a time (32 KiB)
    __shared__ int s_item[3];   // [0], [1]: work items (double-buffered), [2]: chunk_needed flag
    RunBoxes bx;
    int staged = -1;   // template offset whose image is resident in LDS (search_slice)
    if (threadIdx.x == 0) s_item[0] = atomicAdd(queue, 1);
    for (int ph = 0;; ph ^= 1) {
        __syncthreads();                       // one barrier per item: publishes s_item[ph], retires the previous item
        const int item = s_item[ph];
        if (item >= n_work) break;
        if (threadIdx.x == 0) s_item[ph ^ 1] = atomicAdd(queue, 1);   // pop the next item while this one is processed
        const IcpWork wk = work[item];
        const IcpCluster c = cl[wk.cluster];
        const IcpState* sin = st + (size_t)wk.cluster * 2 + (it & 1);          // state before this launch
        const IcpState* snow = st + (size_t)wk.cluster * 2 + ((it + 1) & 1);   // written by k_icp_solve(it)
        if (sin->done) continue;
        const int done_now = snow->done;
        const int q0 = wk.tile * qslice;
        const int nq = min(qslice, c.n - q0);
        float4* pts = src + c.src_off + q0;
        int* nnq = nn + c.src_off + q0;
        float* d2q = d2buf + c.src_off + q0;
        if (it > 0) transform_slice(snow->T, pts, nq);
        if (done_now) continue;
        __syncthreads();   // the transformed points are read by other waves below
        const TplRef t = tpl_ref(tpl, tlo, thi, c.tpl_off);
        QueryRegs q;
        int nk;
        fetch_queries(t.p, c.tpl_m, pts, nq, it > 0, it < 3, false, nullptr, nnq, q, nk);
        search_slice(t, c, grids, q, nk, s_tpl, bx, staged, &s_item[2]);
        store_queries(q, nk, nnq, d2q);
        __syncthreads();
        slice_moments<BOUNDED>(pts, t.p, nnq, d2q, nq, acc, bnd, (size_t)wk.cluster * 3 + it % 3, s_scr);
    }
}

// ---------------------------------------------------------------------------------------
// Persistent form of the sliced driver (few clusters: one frame, small batches).  The multi-launch form above pays two
// dependent kernel launches per PCL iteration (k_icp_solve, k_icp_iter: ~20 us together for one frame, most of it launch
// turnaround); here ONE launch runs every iteration and the fitness pass:
//   * work items (cluster, slice) are assigned statically, item i -> workgroup i % G, so a workgroup meets the same points
//     in every iteration (no other workgroup ever reads them) and stages its template once;
//   * the only data that crosses workgroups are the 16 moment sums of a cluster's correspondences: device-scope atomic adds
//     into acc[cluster][it % 3], read back with device-scope atomic loads after a grid barrier (atomic arrive counter; the
//     barrier inside a workgroup waits for its memory operations first, so no cache-flushing fence is needed);
//   * every workgroup solves (Umeyama + convergence tests) for the clusters of its own items from those sums - a few
//     redundant single-lane solves instead of a second barrier - and keeps their state in LDS; the workgroup that holds
//     slice 0 of a cluster publishes it.
// All G <= n_CU workgroups must be resident together (one per CU): they are, unless other kernels hold the CUs, in which
// case the ones already running wait at the barrier.  Every wait is bounded (2^15 polls, some tens of milliseconds): a
// barrier that does not complete raises the abort flag, every workgroup leaves, and the host runs the multi-launch form instead.
// The slice code is k_icp_iter's and k_icp_fitness's own (transform_slice, search_slice, slice_moments, slice_fitness), the solve
// is icp_step, and the moments are order-free integer sums: identical results.
// ---------------------------------------------------------------------------------------
constexpr int PERSIST_ITEMS = 8;   // work items per workgroup at most

// What crosses workgroups in k_icp_persist are agent-scope atomics only (moment adds, zero-stores, the counters below):
// they are performed at the device's coherence point, so no cache write-back is needed - but they must have been
// PERFORMED before this workgroup counts as arrived.  __syncthreads() alone does not give that on gfx950 (the backend
// emits s_waitcnt lgkmcnt(0) + s_barrier: a workgroup-scope fence does not wait for vector-memory operations outside
// tgsplit mode), so every thread first waits for its own outstanding vector-memory operations (gfx9 counts loads, stores
// and atomics without return in vmcnt alike).  The points / neighbour arrays a workgroup writes with plain stores are only
// ever read back by the same workgroup, hence no agent-scope release fence (which would write the L2 back every iteration).
__device__ __forceinline__ bool grid_barrier(unsigned* bar, unsigned target, int* abort_flag, int* s_ok) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        for (int spins = 0;; ++spins) {
            if (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) break;
            if (spins > (1 << 15) || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
        *s_ok = ok;
    }
    __syncthreads();   // everything after it is issued after thread 0 saw the full count (loads are not hoisted over s_barrier)
    asm volatile("" ::: "memory");
    return *s_ok != 0;
}

#ifdef CD_PERSISTDBG
// time workgroup 0 spends per phase of an iteration (100 MHz ticks): solve, transform, fetch + search + store, moments, barrier
CD_DEBUG_COUNTERS(g_persist_dbg, [8], cd_debug_persist)
#endif
// BOUNDED (rule C8): as k_icp_iter + k_icp_solve - the kept correspondences are counted in bnd.ncorr[cluster][it % 3]
template <bool BOUNDED>
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_persist(int n_work, int max_it, const IcpWork* __restrict__ work,
                                                              const IcpCluster* __restrict__ cl, IcpState* st,
                                                              unsigned long long* acc, unsigned long long* __restrict__ accf,
                                                              const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                              const float4* __restrict__ thi, const IcpGrid* __restrict__ grids,
                                                              float4* src, const float4* __restrict__ src0, int* nn, float* d2buf,
                                                              int qslice, unsigned* bar, int* abort_flag, int n_open, int* closed, IcpParams prm,
                                                              IcpBound bnd) {
    __shared__ float4 s_tpl[ICPT_IMG];
    __shared__ unsigned long long s_scr[8 * ICP_QSLICE];   // moment scratch, 8 terms at a time (32 KiB)
    __shared__ IcpState s_st[PERSIST_ITEMS];               // state of the clusters of this workgroup's items
    __shared__ unsigned long long s_A[16];
    __shared__ int s_flag, s_ok;
    __shared__ uint32_t s_nv;   // (BOUNDED) kept correspondences of the previous iteration
    const int lane = threadIdx.x & 63;
    const int G = gridDim.x;
    int n_items = 0;
    for (int i = blockIdx.x; i < n_work; i += G) ++n_items;   // <= PERSIST_ITEMS (host)
    for (int j = threadIdx.x; j < n_items; j += ICPT_THREADS) s_st[j] = st[2 * (size_t)work[blockIdx.x + j * G].cluster];
    __syncthreads();
    RunBoxes bx;
    int staged = -1;
    bool aborted = false;
#ifdef CD_PERSISTDBG
    unsigned long long tdbg_ = wall_clock64();
#endif
    int it = 0;
    int seen0 = 0, seen1 = 0, seen2 = 0, seen3 = 0;   // closed[0..3] as last read
    for (; it < max_it; ++it) {
        for (int j = 0; j < n_items; ++j) {
            const IcpWork wk = work[blockIdx.x + j * G];
            const IcpCluster c = cl[wk.cluster];
            const bool was_done = s_st[j].done != 0;   // uniform: LDS value written before the last barrier
            if (was_done) continue;
            if (it > 0) {   // this iteration's transformation from the previous iteration's correspondences
                if (threadIdx.x < 16)
                    s_A[threadIdx.x] = __hip_atomic_load(acc + ((size_t)wk.cluster * 3 + (it - 1) % 3) * 16 + threadIdx.x, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                if (BOUNDED && threadIdx.x == 16)
                    s_nv = __hip_atomic_load(bnd.ncorr + (size_t)wk.cluster * 3 + (it - 1) % 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __syncthreads();
                if (threadIdx.x == 0) {
                    IcpState so = s_st[j];
                    so.done = icp_step<BOUNDED>(so, s_A, BOUNDED ? (int)s_nv : c.n, prm);
                    s_st[j] = so;
                    // one count per cluster that closes in iteration `it`, into the slot of that iteration (see the exit test)
                    if (wk.tile == 0 && so.done) __hip_atomic_fetch_add(closed + (it & 3), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
            }
            PERSIST_PHASE(0)
            if (wk.tile == 0 && threadIdx.x < 16)   // the sums of iteration it + 1 start from zero (slot last read in iteration it - 1)
                __hip_atomic_store(acc + ((size_t)wk.cluster * 3 + (it + 1) % 3) * 16 + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (BOUNDED && wk.tile == 0 && threadIdx.x == 16)
                __hip_atomic_store(bnd.ncorr + (size_t)wk.cluster * 3 + (it + 1) % 3, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int done_now = s_st[j].done;
            const int q0 = wk.tile * qslice;
            const int nq = min(qslice, c.n - q0);
            float4* pts = src + c.src_off + q0;
            int* nnq = nn + c.src_off + q0;
            float* d2q = d2buf + c.src_off + q0;
            if (it > 0) transform_slice(s_st[j].T, pts, nq);
            if (done_now) continue;
            __syncthreads();   // the transformed points are read by other waves below
            PERSIST_PHASE(1)
            const TplRef t = tpl_ref(tpl, tlo, thi, c.tpl_off);
            QueryRegs q;
            int nk;
            fetch_queries(t.p, c.tpl_m, pts, nq, it > 0, it < 3, false, nullptr, nnq, q, nk);
            search_slice(t, c, grids, q, nk, s_tpl, bx, staged, &s_flag);
            store_queries(q, nk, nnq, d2q);
            __syncthreads();
            PERSIST_PHASE(2)
            slice_moments<BOUNDED>(pts, t.p, nnq, d2q, nq, acc, bnd, (size_t)wk.cluster * 3 + it % 3, s_scr);
            __syncthreads();   // s_scr is reused by the next item
            PERSIST_PHASE(3)
        }
        if (!grid_barrier(bar, (unsigned)(it + 1) * (unsigned)G, abort_flag, &s_ok)) { aborted = true; break; }
        PERSIST_PHASE(4)
        // Exit when every cluster has closed - decided from state that is FINAL at this barrier: closed[it & 3] only receives
        // the closes of iterations it, it - 4, ... (a workgroup that runs ahead adds to slot (it + 1) & 3, and slot it & 3 is
        // next written in iteration it + 4, which nobody enters before all have left barrier it + 3), and every workgroup
        // reads slot it & 3 between barrier it and its arrival at barrier it + 1.  All workgroups therefore see the same
        // running total and leave in the same iteration.  (A single shared count of open clusters was read "from the
        // future": a slower workgroup could see the zero a faster one produced one iteration later and leave early.)
        {
            const int v = __hip_atomic_load(closed + (it & 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen0 = (it & 3) == 0 ? v : seen0; seen1 = (it & 3) == 1 ? v : seen1;
            seen2 = (it & 3) == 2 ? v : seen2; seen3 = (it & 3) == 3 ? v : seen3;
        }
        if (seen0 + seen1 + seen2 + seen3 >= n_open) { ++it; break; }
    }
    if (aborted) return;
    // fitness pass and publication of the states
    for (int j = 0; j < n_items; ++j) {
        const IcpWork wk = work[blockIdx.x + j * G];
        const IcpCluster c = cl[wk.cluster];
        if (wk.tile == 0 && threadIdx.x == 0) { st[2 * (size_t)wk.cluster] = s_st[j]; st[2 * (size_t)wk.cluster + 1] = s_st[j]; }
        if (s_st[j].status != CD_OK) continue;
        float T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = s_st[j].Tfinal[k];
        const int q0 = wk.tile * qslice;
        const int nq = min(qslice, c.n - q0);
        __syncthreads();
        const unsigned long long v = wave_sum_u64(slice_fitness(tpl_ref(tpl, tlo, thi, c.tpl_off), c, grids, T, src0 + c.src_off + q0, nq,
                                                                nn + c.src_off + q0, d2buf + c.src_off + q0, s_tpl, bx, staged, &s_flag));
        if (lane == 0 && v) atomicAdd(&accf[wk.cluster], v);
    }
}

// getFitnessScore(): mean squared NN distance of T_final * (original source)
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_fitness(const IcpWork* __restrict__ work,
                                                              const IcpCluster* __restrict__ cl,
                                                              const IcpState* __restrict__ st, int parity,
                                                              unsigned long long* __restrict__ accf,
                                                              const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                              const float4* __restrict__ thi, const IcpGrid* __restrict__ grids,
                                                              const float4* src0, int* nn, float* d2buf, int qslice) {
    __shared__ float4 s_tpl[ICPT_IMG];
    __shared__ unsigned long long s_acc;
    __shared__ float s_T[16];
    __shared__ int s_flag;
    const IcpWork wk = work[blockIdx.x];
    const IcpCluster c = cl[wk.cluster];
    const IcpState* s = st + (size_t)wk.cluster * 2 + parity;
    if (s->status != CD_OK) return;
    if (threadIdx.x < 16) s_T[threadIdx.x] = s->Tfinal[threadIdx.x];
    if (threadIdx.x == 16) s_acc = 0ull;
    __syncthreads();
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = s_T[k];
    const int q0 = wk.tile * qslice;
    const int nq = min(qslice, c.n - q0);
    RunBoxes bx;
    int staged = -1;   // one item per workgroup: nothing is resident yet
    const unsigned long long v = slice_fitness(tpl_ref(tpl, tlo, thi, c.tpl_off), c, grids, T, src0 + c.src_off + q0, nq, nn + c.src_off + q0,
                                               d2buf + c.src_off + q0, s_tpl, bx, staged, &s_flag);
    if ((threadIdx.x & ~63) < nq) {
        const unsigned long long t = wave_sum_u64(v);
        if ((threadIdx.x & 63) == 0) atomicAdd(&s_acc, t);
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&accf[wk.cluster], s_acc);
}

// pcl::Registration::align(output, guess): input_transformed = guess * source before the first iteration (the iterations
// then run on d_src as they do from the identity; final_transformation_ starts as the guess - the host puts it into the
// initial IcpState).  guesses: one row-major 4x4 per frame (per_frame == 1), per ICP problem (per_frame == 2: CD_GUESS_CLUSTER,
// written by k_shape_frames) or a single one (per_frame == 0).
__global__ void __launch_bounds__(BLOCK) k_icp_apply_guess(const IcpCluster* __restrict__ cl, const float* __restrict__ guesses,
                                                           int per_frame, const float4* __restrict__ src0, float4* __restrict__ src) {
    const IcpCluster c = cl[blockIdx.x];
    const float* G = guesses + (per_frame == 2 ? 16 * (size_t)blockIdx.x : (per_frame ? 16 * (size_t)c.frame : 0));
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = G[k];
    for (int i = blockIdx.y * BLOCK + threadIdx.x; i < c.n; i += gridDim.y * BLOCK) {
        const float4 p = src0[c.src_off + i];
        float ox, oy, oz;
        xform(T, p.x, p.y, p.z, ox, oy, oz);
        src[c.src_off + i] = make_float4(ox, oy, oz, p.w);
    }
}
void launch_icp_apply_guess(hipStream_t s, int ncl, int max_n, const IcpCluster* cl, const float* guesses, int per_frame,
                            const float4* src0, float4* src) {
    if (ncl <= 0 || max_n <= 0) return;
    const int gx = (max_n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_icp_apply_guess, dim3(ncl, gx < 64 ? gx : 64), dim3(BLOCK), 0, s, cl, guesses, per_frame, src0, src);
}

void launch_icp_iter(hipStream_t s, int it, int n_work, int ncl, const IcpWork* work, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                     int qslice, int n_cu, IcpParams prm, const IcpBound& bnd) {
    if (ncl <= 0) return;
    if (bnd.bounded) hipLaunchKernelGGL(k_icp_solve<true>, dim3((ncl + WAVE - 1) / WAVE), dim3(WAVE), 0, s, it, ncl, P.cl, P.st, S.acc, S.queue, prm, bnd);
    else hipLaunchKernelGGL(k_icp_solve<false>, dim3((ncl + WAVE - 1) / WAVE), dim3(WAVE), 0, s, it, ncl, P.cl, P.st, S.acc, S.queue, prm, bnd);
    if (n_work <= 0) return;   // every cluster converged: only the state bookkeeping above is needed
    if (bnd.bounded)
        hipLaunchKernelGGL(k_icp_iter<true>, dim3(n_work < n_cu ? n_work : n_cu), dim3(ICPT_THREADS), 0, s, it, n_work, work, P.cl, P.st, S.acc, T.tplk, T.tlok,
                           T.thik, T.grids, S.src, S.nn, S.d2, qslice, S.queue, bnd);
    else
        hipLaunchKernelGGL(k_icp_iter<false>, dim3(n_work < n_cu ? n_work : n_cu), dim3(ICPT_THREADS), 0, s, it, n_work, work, P.cl, P.st, S.acc, T.tplk, T.tlok,
                           T.thik, T.grids, S.src, S.nn, S.d2, qslice, S.queue, bnd);
}
void launch_icp_fitness(hipStream_t s, int n_work, const IcpWork* work, const IcpProblems& P, int parity, const IcpTemplates& T, const IcpScratch& S, int qslice) {
    if (n_work <= 0) return;
    hipLaunchKernelGGL(k_icp_fitness, dim3(n_work), dim3(ICPT_THREADS), 0, s, work, P.cl, P.st, parity, P.accf, T.tplk, T.tlok, T.thik, T.grids, S.src0, S.nn, S.d2, qslice);
}

void launch_icp_persist(hipStream_t s, int n_work, int n_wg, int max_it, const IcpWork* work, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                        int qslice, unsigned* bar, int* abort_flag, int n_open, int* closed, IcpParams prm, const IcpBound& bnd) {
    if (n_work <= 0 || n_wg <= 0) return;
    hipLaunchKernelGGL(bnd.bounded ? k_icp_persist<true> : k_icp_persist<false>, dim3(n_wg), dim3(ICPT_THREADS), 0, s, n_work, max_it, work, P.cl, P.st, S.acc, P.accf,
                       T.tplk, T.tlok, T.thik, T.grids, S.src, S.src0, S.nn, S.d2, qslice, bar, abort_flag, n_open, closed, prm, bnd);
}

}  // namespace cd
