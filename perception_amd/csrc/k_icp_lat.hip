// k_icp_lat.hip - S6 point-to-point ICP against a LATTICE template: closed-form nearest neighbour.
//
// Replaces pcl::IterativeClosestPoint<PointXYZ,PointXYZ>::align + getFitnessScore (reference:
// cuboid_detection/src/iterative_closest_point.cpp:170-182, object_detection/src/object_pose_detection.cpp:220-235) for the
// templates cuboid_detection/templates/make_cuboid.py:38-55 writes: face k = meshgrid of two of the three axis tables
// X, Y, Z at a constant third coordinate, first axis fastest, faces one after the other.  cd_set_template verifies that
// structure bit by bit against the uploaded points (lattice_detect, template_prep.hpp) and hands over IcpLattice (common.hpp);
// every other template keeps the pruned searches of icp_search.hpp and k_icp_pipe.hip.
//
// The search.  The canonical squared distance (rule C1/C5, common.hpp dist2) to point (i, j) of a face with constant z = c is
//     d2(i, j) = fl(fl(fx(i) + fy(j)) + fz),   fx(i) = fl(fl(qx - X[i])^2),  fy(j) = fl(fl(qy - Y[j])^2),  fz = fl(fl(qz - c)^2)
// (the constant term takes the place of its axis for the faces of constant x or y).  Every rounded operation is monotone:
// fl(a + b) does not decrease when a or b grows, fl(q - t) does not increase when t grows, squaring is monotone in |.|.  Hence
//   (1) min over the face = d2(i*, j*) with i* = argmin fx, j* = argmin fy - the two axes separate;
//   (2) fx is unimodal in i (tables ascend), so i* is the table entry nearest to qx: with tables uniform to 1/16 of a step
//       (verified on the host) it is one of ig - 1, ig, ig + 1 for ig = clamp(rint((qx - X[0]) / step)), all three evaluated
//       exactly - one 16-byte LDS read of the window (X[ig-1], X[ig], X[ig+1]);
//   (3) the points of the face that TIE with the minimum (equal float d2; rule C5 wants the lowest original index =
//       lowest slow-axis index, then lowest fast-axis index) form, along each axis, a contiguous run that contains i* / j*:
//       walk the slow axis down while d2(i*, j - 1) == min, then the fast axis.  A tie needs f(lower neighbour) - f(min) below
//       the rounding of the sum, so the walk is only entered by lanes whose gap is <= 2^-21 * min (a conservative filter:
//       it only ever sends too many lanes to the exact test);
//   (4) faces are consecutive in the file, so across faces the lexicographic (d2, index) minimum is the FIRST face that
//       reaches the minimum.
// Checked against brute force with the oracle's arithmetic on all five reference cuboid templates incl. the 21 400-point
// six-face one: tests/test_gpu_lattice.py (near, far, mid-cell, +-300 m along a face normal - a tie walk across the whole face).
// ~215 vector instructions per pass of 64 queries (transform 18, three axes 51, faces 52, tie filter 13, moment terms 67, loop 14),
// no divergence outside the rare tie walk, against ~2400 per pass of the pruned searches - and no 116 KB template image: a slot
// needs 8.7 KB of LDS, so ICP workgroups stop monopolising CUs.
//
// Launch shape: a workgroup keeps one or several clusters going, every cluster's whole ICP inside it (k_icp_lat<CPW, WPC> below).
// No MFMA: there is no dense contraction here (3x3 matrices only).
#include "kernels.hpp"
#include "icp_solve_row.hpp"
#include "lat_search.hpp"

namespace cd {

// ---------------------------------------------------------------------------------------------------------------------------
// k_icp_lat<CPW, WPC>: a workgroup keeps CPW clusters ("slots") going, WPC waves each, and works in ROUNDS of two phases:
//   work  : the waves of a slot take the passes (64 points each) of the slot's current step - a PCL iteration (X <- T X in
//           place, nearest neighbours, the 16 fixed-point moment sums of rule C4 kept in registers and folded into the slot's
//           LDS accumulators) or, once converged, the final transform + getFitnessScore() pass;            -- barrier --
//   solve : a row of 16 lanes per slot (row s % 4 of wave s / 4) finishes the slot's step: Umeyama + SVD + convergence tests
//           (icp_step_row, icp_solve_row.hpp: icp_step - what every other driver calls on one lane - spread over the row, the
//           same bits), or the row's first lane writes a finished cluster back and refills the slot from the launch's cluster
//           queue.  The solves of a workgroup's slots run SIDE BY SIDE in the rows of one or two waves.      -- barrier --
// Why this shape (measured, tools/lat_threads_serial.sh, tools/probe_lat_phases.py): a step of a 1 400-point cluster is ~19 us
// of passes for one wave, and its solve was ~13 k cycles on a single lane (3 300 dependent instructions: IEEE divisions and
// square roots of the Jacobi sweeps, 17 double divisions before them, two 4x4 products after).  The row does the elementwise
// parts once per lane instead of once per entry and the sweeps' square roots and reciprocals in exact shorter forms; the
// rotation parameters remain a serial chain that every lane of the row repeats (profiles/EXPERIMENTS.md A11 for the cycles).
// One cluster per workgroup of four waves still spends close to half of its life with its waves parked behind that chain; CPW
// clusters per workgroup pay it once per round for all of them.  <1, 4> / <1, 16> (one cluster, many waves) remain the
// latency shapes: a launch that has the GPU to itself, a single frame.
// Each slot has its own copy of its template's tables (a launch may mix templates: BASELINE config 5), restaged when a refill
// brings a cluster of another template.
// ---------------------------------------------------------------------------------------------------------------------------
#ifdef CD_LAT_TIMERS
// phase times of k_icp_lat, summed over workgroups (thread 0's clock64 cycles): [0] work phase, [1] wait at the barrier after it,
// [2] solve phase, [3] wait at the barrier after it, [4] rounds, [5] staging
__device__ unsigned long long g_lat_stats[8];
extern "C" int cd_debug_lat_stats(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lat_stats), sizeof(g_lat_stats)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lat_stats), z, sizeof(z)); }
    return 0;
}
#define LAT_T(k) { const long long tn_ = clock64(); tph[k] += tn_ - tlast; tlast = tn_; }
#else
#define LAT_T(k)
#endif

// (LatFaces, lat_nearest, lat_nearest_axes, the tie walk and LatFix: lat_search.hpp.  The queue pop, the table staging, the search
// dispatch, the two-branch accumulate, the pass loop's head and the fitness pass below are this kernel's OWN text of
// icp_pop_live, lat_stage_tables, lat_nearest_any, lat_fix_terms, lat_for_passes and lat_fitness_pass: each of the six, taken
// alone, changes the code of the 26 instantiations - lat_fix_terms puts them into scratch (profiles/EXPERIMENTS.md) - and this
// is the kernel the benchmark times.  A fix to one of those helpers is made here too.)
struct LatSlot {
    int k, src_off, n, tslot;   // the cluster (index, first point, points, template slot)
    int phase;                  // LAT_ITER / LAT_FIT / LAT_EMPTY
    int gen;                    // bumped by every refill: the slot's waves restage tables and face descriptors
    int ready;                  // the work phase of this round added a step's sums
    int pad;
};
enum { LAT_ITER = 0, LAT_FIT = 1, LAT_EMPTY = 2 };

#ifndef CD_LAT_SOLVE_ROW
#define CD_LAT_SOLVE_ROW 1   // 0: the single-lane icp_step in the solve phase (variant builds, A/B)
#endif
#ifndef CD_LAT_WAVES_PER_EU
#define CD_LAT_WAVES_PER_EU 4   // four waves per SIMD: 128 registers (the pass loop and the solve both need more than 96)
#endif
// BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter the sums; s_nv counts them per slot (one popcount of a
// ballot per pass and wave, one LDS add per wave and round) and takes the place of n in the solve and in the constants' offset
template <int CPW, int WPC, bool BOUNDED>
__global__ void __launch_bounds__(CPW * WPC * WAVE, CD_LAT_WAVES_PER_EU)
k_icp_lat(int nitems, const int* __restrict__ order, const IcpCluster* __restrict__ cl, IcpState* __restrict__ st,
          unsigned long long* __restrict__ accf, const IcpLattice* __restrict__ lats, float4* __restrict__ src,
          const float4* __restrict__ src0, int* __restrict__ queue, unsigned long long* __restrict__ busy,
          unsigned long long* __restrict__ busy_out, IcpParams prm, IcpBound bnd) {
    // (order / cl / st / accf may be the host's pinned arrays: every access to them is one cluster's record at a refill or at
    // the end of its ICP.  busy_out != nullptr: the last workgroup to finish writes the launch's wave-time there - queue[1]
    // counts the finished workgroups)
    __shared__ float4 s_tab[CPW][LAT_MAX_TAB];
    __shared__ int4 s_face[CPW][2 * LAT_MAX_FACES];
    __shared__ unsigned long long s_acc[CPW][16];
    __shared__ IcpState s_so[CPW];
    __shared__ LatSlot s_slot[CPW];
    __shared__ int s_flags[2];   // [0] always 0 (see the solve phase), [1] some slot was refilled in this round
    __shared__ unsigned s_nv[BOUNDED ? CPW : 1];   // (BOUNDED) kept correspondences of the slot's current step
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = wave / WPC, sub = wave % WPC;
    const long long wg_t0 = wall_clock64();   // (100 MHz: the workgroup's lifetime goes to accf[nitems_all], see the end)
    // refill of slot s by one lane: the next live cluster of the queue (largest first), or nothing left
    auto refill = [&](int s) {
        LatSlot& sl = s_slot[s];
        for (int i = 0; i < 16; ++i) s_acc[s][i] = 0ull;
        if constexpr (BOUNDED) s_nv[s] = 0u;
        sl.ready = 0;
        for (;;) {
            const int item = atomicAdd(queue, 1);
            if (item >= nitems) { sl.phase = LAT_EMPTY; return; }
            const int k = order[item];
            if (st[2 * (size_t)k].done) continue;   // host pre-marked (too few points / no template)
            const IcpCluster c = cl[k];
            sl.k = k; sl.src_off = c.src_off; sl.n = c.n; sl.tslot = c.slot;
            s_so[s] = st[2 * (size_t)k];
            sl.phase = LAT_ITER;
            sl.gen += 1;
            return;
        }
    };
    if (threadIdx.x < CPW) { s_slot[threadIdx.x].gen = 0; refill(threadIdx.x); }
    if (threadIdx.x == 0) { s_flags[0] = 0; s_flags[1] = 1; }
    __syncthreads();
    int my_gen = 0;
#ifdef CD_LAT_TIMERS
    long long tph[6] = {0, 0, 0, 0, 0, 0}, tlast = clock64();
#endif
    for (;;) {
        if (s_flags[1]) {   // (uniform) some slot has a new cluster: its waves stage the tables of the cluster's template
            const LatSlot sl = s_slot[slot];
            const bool mine = sl.phase != LAT_EMPTY && sl.gen != my_gen;
            if (mine) {
                const IcpLattice* __restrict__ L = lats + sl.tslot;
                for (int i = sub * WAVE + lane; i < L->ntab; i += WPC * WAVE) s_tab[slot][i] = L->tab[i];
                if (sub == 0 && lane < LAT_MAX_FACES) {
                    const int f = lane, w = L->w[f], u = L->fast[f], v = 3 - w - u;
                    s_face[slot][f] = make_int4(w, u, L->base[f], __float_as_int(L->c[f]));
                    s_face[slot][LAT_MAX_FACES + f] = make_int4(L->toff[u], L->toff[v < 0 || v > 2 ? 0 : v], L->n[u], 0);
                }
                my_gen = sl.gen;
            }
            __syncthreads();
        }
        LAT_T(5)
        // ---- work phase ----
        {
            // (the slot's words as scalars; the face words of its template are re-read every round - a few scalar loads that hit
            // the constant cache - rather than carried across the solve phase in forty scalar registers)
            const int phase = __builtin_amdgcn_readfirstlane(s_slot[slot].phase), n = __builtin_amdgcn_readfirstlane(s_slot[slot].n);
            const int src_off = __builtin_amdgcn_readfirstlane(s_slot[slot].src_off), tslot = __builtin_amdgcn_readfirstlane(s_slot[slot].tslot);
            const int npass = (n + 63) >> 6;
            float4* pts = src + src_off;
            const float4* tab = s_tab[slot];
            const int4* face = s_face[slot];
            LatFaces F;
            {
                const IcpLattice* __restrict__ L = lats + (phase == LAT_EMPTY ? 0 : tslot);
                lat_faces_load(L, F);
            }
            const bool nf3 = F.nface <= 3;
            if (phase == LAT_ITER) {
                const bool moved = s_so[slot].iters > 0;   // X <- T*X from the second iteration on
                float T[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) T[i] = s_so[slot].T[i];   // (uniform values in vector registers: as scalars they were spilled and re-read lane by lane in every pass)
                unsigned long long S[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) S[i] = 0ull;
                unsigned nv = 0u;   // (BOUNDED: kept correspondences of this wave's passes, wave-uniform)
                // (the points of the next pass are requested before the current pass is worked on: one wave per SIMD per cluster has
                // nothing else to cover an L2 round trip with)
                float4 pnext = pts[min((sub << 6) + lane, n - 1)];
                for (int pss = sub; pss < npass; pss += WPC) {
                    const int myq = (pss << 6) + lane;
                    const bool act = myq < n;
                    const float4 p = pnext;
                    pnext = pts[min(((pss + WPC) << 6) + lane, n - 1)];
                    float px = p.x, py = p.y, pz = p.z;
                    if (moved) {   // written back by the lane that owns the point
                        xform(T, p.x, p.y, p.z, px, py, pz);
                        if (act) pts[myq] = make_float4(px, py, pz, p.w);
                    }
                    const LatHit h = F.axes ? lat_nearest_axes<true>(tab, face, F, px, py, pz)
                                            : (nf3 ? lat_nearest<true, 3>(tab, face, F, px, py, pz) : lat_nearest<true, LAT_MAX_FACES>(tab, face, F, px, py, pz));
                    // the 16 moment terms of rule C4, accumulated as raw bits (LatFix above: the solver takes the constants off
                    // again).  Valid while every term stays below 2^50 / 2^shift; a point outside that range (coordinates beyond
                    // 256 m, a neighbour more than 128 m away) takes the general conversion - the same integers either way.  Lanes
                    // without a point add nothing; BOUNDED: nor do lanes whose correspondence is rejected (rule C8).
                    const bool keep = act && (!BOUNDED || h.d <= bnd.d2_max);
                    if constexpr (BOUNDED) nv += (unsigned)__popcll(ballot64(keep));
                    if (keep) {
                        const float pv[3] = {px, py, pz}, qv[3] = {h.nx, h.ny, h.nz};
                        const float big_c = fmaxf(fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)), fmaxf(fmaxf(fabsf(h.nx), fabsf(h.ny)), fabsf(h.nz)));
                        if (big_c < 256.f && h.d < 16384.f) {
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                S[a] += LatFix<FIX_SHIFT>::bits(pv[a]);
                                S[3 + a] += LatFix<FIX_SHIFT>::bits(qv[a]);
#pragma unroll
                                for (int b = 0; b < 3; ++b) S[6 + 3 * a + b] += LatFix<FIX_SHIFT>::bits(__fmul_rn(qv[a], pv[b]));
                            }
                            S[15] += LatFix<FIX_SHIFT_D2>::bits(h.d);
                        } else {
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                S[a] += LatFix<FIX_SHIFT>::general(pv[a]);
                                S[3 + a] += LatFix<FIX_SHIFT>::general(qv[a]);
#pragma unroll
                                for (int b = 0; b < 3; ++b) S[6 + 3 * a + b] += LatFix<FIX_SHIFT>::general(__fmul_rn(qv[a], pv[b]));
                            }
                            S[15] += LatFix<FIX_SHIFT_D2>::general(h.d);
                        }
                    }
                }
                if (sub < npass) wave_fold_to_lds(S, 16, s_acc[slot]);
                if constexpr (BOUNDED) { if (sub < npass && lane == 0) atomicAdd(&s_nv[slot], nv); }
                if (sub == 0 && lane == 0) s_slot[slot].ready = 1;
            } else if (phase == LAT_FIT) {
                // final X <- T*X (PCL transforms before it tests convergence), then getFitnessScore() of Tfinal * original source
                const float4* pts0 = src0 + src_off;
                float T[12], Tf[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    T[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_so[slot].T[i])));
                    Tf[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_so[slot].Tfinal[i])));
                }
                unsigned long long S[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) S[i] = 0ull;
                float4 pnext = pts[min((sub << 6) + lane, n - 1)], p0next = pts0[min((sub << 6) + lane, n - 1)];
                for (int pss = sub; pss < npass; pss += WPC) {
                    const int myq = (pss << 6) + lane;
                    const bool act = myq < n;
                    const float4 p = pnext, p0 = p0next;
                    pnext = pts[min(((pss + WPC) << 6) + lane, n - 1)];
                    p0next = pts0[min(((pss + WPC) << 6) + lane, n - 1)];
                    float ox, oy, oz;
                    xform(T, p.x, p.y, p.z, ox, oy, oz);
                    if (act) pts[myq] = make_float4(ox, oy, oz, p.w);
                    float qx, qy, qz;
                    xform(Tf, p0.x, p0.y, p0.z, qx, qy, qz);
                    const LatHit h = F.axes ? lat_nearest_axes<false>(tab, face, F, qx, qy, qz)
                                            : (nf3 ? lat_nearest<false, 3>(tab, face, F, qx, qy, qz) : lat_nearest<false, LAT_MAX_FACES>(tab, face, F, qx, qy, qz));
                    if (act) S[0] += lat_fix_d2(h.d);
                }
                if (sub < npass) wave_fold_to_lds(S, 1, s_acc[slot]);
            }
        }
        LAT_T(0)
        // (every thread has read s_flags[1] for this round - those that found it set have also passed the staging barrier - and
        // nobody raises it before the barrier below)
        if (threadIdx.x == 0) s_flags[1] = 0;
        __syncthreads();
        LAT_T(1)
#if CD_LAT_SOLVE_ROW
        // ---- solve phase: slot s <-> the row of 16 lanes 16 * (s % 4) .. + 15 of wave s / 4 (CPW <= 4: wave 0; CPW = 8: waves 0
        // and 1).  The row solves the slot's step together (icp_step_row); write-back, refill and the slot's words stay with the
        // row's first lane.  (s_flags[1] was cleared before the barrier above: two waves may raise it here) ----
        // tid: the thread index through a zero read from LDS in every round.  The compiler cannot move what the row derives from
        // it (lane numbers, the addresses of the slot's state and sums) out of the round loop, where a dozen such values would
        // stay in registers across the pass loop and push it into scratch.  Nothing but the compiler's ignorance of that zero keeps
        // it so: tests/test_lat_loop_count.py (no spill, no scratch, <= 128 VGPRs in all 26 instantiations) is what holds it.
        const int tid = (int)threadIdx.x | s_flags[0];
        if (tid < CPW * 16) {
            const int s = tid >> 4, l = tid & 15;
            LatSlot& sl = s_slot[s];
            const int phase = sl.phase, ready = sl.ready;
            // (every point added the constant of its scale to each sum it touched: see LatFix; BOUNDED: every KEPT point, and
            // the fitness pass below keeps them all)
            const int nv = BOUNDED && phase == LAT_ITER ? (int)s_nv[s] : sl.n;
            const unsigned long long off = (unsigned long long)nv * LatFix<FIX_SHIFT>::C, off_d = (unsigned long long)nv * LatFix<FIX_SHIFT_D2>::C;
            if (phase == LAT_ITER && ready) {
                RowLanes row(tid);
                RowLanes::V<unsigned long long> a;
                a.v = s_acc[s][l] - (l == 15 ? off_d : off);   // the lane that owns a sum takes the constants off it
                const int done = icp_step_row<BOUNDED>(row, s_so[s], a, nv, prm);
                s_acc[s][l] = 0ull;
                if (l == 0) {
                    if (done) sl.phase = LAT_FIT;
                    if constexpr (BOUNDED) s_nv[s] = 0u;
                    sl.ready = 0;
                }
            } else if (phase == LAT_FIT && l == 0) {
                s_so[s].done = 1;
                st[2 * (size_t)sl.k] = s_so[s];
                st[2 * (size_t)sl.k + 1] = s_so[s];
                accf[sl.k] = s_acc[s][0] - off_d;
                refill(s);
                if (sl.phase != LAT_EMPTY) s_flags[1] = 1;
            }
        }
#else
        // ---- solve phase, single-lane variant (-DCD_LAT_SOLVE_ROW=0, A/B runs): lane s of wave 0 <-> slot s ----
        if (threadIdx.x < CPW) {
            const int s = threadIdx.x;
            LatSlot& sl = s_slot[s];
            const int nv = BOUNDED && sl.phase == LAT_ITER ? (int)s_nv[s] : sl.n;
            const unsigned long long off = (unsigned long long)nv * LatFix<FIX_SHIFT>::C, off_d = (unsigned long long)nv * LatFix<FIX_SHIFT_D2>::C;
            if (sl.phase == LAT_ITER && sl.ready) {
                for (int i = 0; i < 15; ++i) s_acc[s][i] -= off;
                s_acc[s][15] -= off_d;
                if (icp_step<BOUNDED>(s_so[s], s_acc[s], nv, prm)) sl.phase = LAT_FIT;
                for (int i = 0; i < 16; ++i) s_acc[s][i] = 0ull;
                if constexpr (BOUNDED) s_nv[s] = 0u;
                sl.ready = 0;
            } else if (sl.phase == LAT_FIT) {
                s_so[s].done = 1;
                st[2 * (size_t)sl.k] = s_so[s];
                st[2 * (size_t)sl.k + 1] = s_so[s];
                accf[sl.k] = s_acc[s][0] - off_d;
                refill(s);
                if (sl.phase != LAT_EMPTY) s_flags[1] = 1;
            }
        }
#endif
        LAT_T(2)
        __syncthreads();
        LAT_T(3)
#ifdef CD_LAT_TIMERS
        tph[4] += 1;
#endif
        // (behind the barrier: the slots of both solving waves are settled, and nobody changes one before the next barrier)
        int all_empty = 1;
#pragma unroll
        for (int s = 0; s < CPW; ++s) all_empty &= s_slot[s].phase == LAT_EMPTY ? 1 : 0;
        if (all_empty) break;
    }
#ifdef CD_LAT_TIMERS
    if (threadIdx.x == 0) for (int i = 0; i < 6; ++i) atomicAdd(&g_lat_stats[i], (unsigned long long)tph[i]);
#endif
    // the wave-time this launch cost: lifetime of the workgroup (100 MHz ticks) x its waves, summed over the workgroups
    // (cd_timing.icp_wave_ms: what a batch's ICP holds of the chip's wave slots, the throughput roof with batches in flight)
    if (threadIdx.x == 0 && busy) {
        atomicAdd(busy, (unsigned long long)(wall_clock64() - wg_t0) * (unsigned long long)(CPW * WPC));
        if (busy_out) {
            __threadfence();
            if (atomicAdd(queue + 1, 1) == (int)gridDim.x - 1) {
                __threadfence();
                *busy_out = atomicAdd(busy, 0ull);
            }
        }
    }
}

__device__ __forceinline__ bool lat_same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// diagnostic / test entry: nearest template point of arbitrary queries (original index and canonical d2)
__global__ void __launch_bounds__(BLOCK) k_lat_nn(const IcpLattice* __restrict__ L, const float4* __restrict__ q, int n, int* __restrict__ out_idx,
                                                  float* __restrict__ out_d2) {
    __shared__ float4 s_tab[LAT_MAX_TAB];
    __shared__ int4 s_face[2 * LAT_MAX_FACES];
    LatFaces F;
    lat_stage<BLOCK>(L, F, s_tab, s_face);
    for (int base = blockIdx.x * BLOCK; base < n; base += gridDim.x * BLOCK) {   // (whole waves stay together: ballots inside)
        const int i = base + threadIdx.x;
        const float4 p = q[i < n ? i : n - 1];
        const LatHit h = lat_nearest<true, LAT_MAX_FACES, true>(s_tab, s_face, F, p.x, p.y, p.z);
        const LatHit g = lat_nearest<false, 3>(s_tab, s_face, F, p.x, p.y, p.z);   // (the three-face form: equal d only when nface <= 3)
        bool same = F.nface > 3 || h.d == g.d;
        const int idx = lat_index(s_face, F, h);
        if (F.axes) {   // (uniform) the one-face-per-axis forms: the same index and distance, or d2 reads NaN
            const LatHit a = lat_nearest_axes<true, true>(s_tab, s_face, F, p.x, p.y, p.z);
            const LatHit b = lat_nearest_axes<false>(s_tab, s_face, F, p.x, p.y, p.z);
            same = same && a.d == h.d && b.d == h.d && lat_same_bits(a.nx, h.nx) && lat_same_bits(a.ny, h.ny) && lat_same_bits(a.nz, h.nz) &&
                   lat_index(s_face, F, a) == idx;
        }
        if (i < n) { out_idx[i] = idx; out_d2[i] = same ? h.d : __uint_as_float(0x7fc00000u); }
    }
}

// shape = clusters per workgroup * 256 + waves per cluster (1 | 2 | 4 | 8 x 1 | 2 | 4 | 8 | 16, at most 16 waves per workgroup)
template <int CPW, int WPC>
static void launch_lat_shape(hipStream_t s, int nitems, int n_wg, const int* order, const IcpCluster* cl, IcpState* st, unsigned long long* accf,
                             const IcpLattice* lats, float4* src, const float4* src0, int* queue, unsigned long long* busy, unsigned long long* busy_out,
                             IcpParams prm, const IcpBound& bnd) {
    if (bnd.bounded)
        hipLaunchKernelGGL((k_icp_lat<CPW, WPC, true>), dim3(n_wg), dim3(CPW * WPC * WAVE), 0, s, nitems, order, cl, st, accf, lats, src, src0, queue, busy, busy_out, prm, bnd);
    else
        hipLaunchKernelGGL((k_icp_lat<CPW, WPC, false>), dim3(n_wg), dim3(CPW * WPC * WAVE), 0, s, nitems, order, cl, st, accf, lats, src, src0, queue, busy, busy_out, prm, bnd);
}
void launch_icp_lat(hipStream_t s, int nitems, int cpw, int wpc, int n_wg, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S,
                    unsigned long long* busy, unsigned long long* busy_out, IcpParams prm, const IcpBound& bnd) {
    if (nitems <= 0 || n_wg <= 0) return;
#define CD_LAT_CASE(C, W) if (cpw == C && wpc == W) return launch_lat_shape<C, W>(s, nitems, n_wg, P.order, P.cl, P.st, P.accf, T.lats, S.src, S.src0, S.queue, busy, busy_out, prm, bnd);
    CD_LAT_CASE(1, 1) CD_LAT_CASE(1, 2) CD_LAT_CASE(1, 4) CD_LAT_CASE(1, 8) CD_LAT_CASE(1, 16)
    CD_LAT_CASE(2, 1) CD_LAT_CASE(2, 2) CD_LAT_CASE(2, 4)
    CD_LAT_CASE(4, 1) CD_LAT_CASE(4, 2) CD_LAT_CASE(4, 4)
    CD_LAT_CASE(8, 1) CD_LAT_CASE(8, 2)
#undef CD_LAT_CASE
    launch_lat_shape<1, 4>(s, nitems, n_wg, P.order, P.cl, P.st, P.accf, T.lats, S.src, S.src0, S.queue, busy, busy_out, prm, bnd);
}
void launch_lat_nn(hipStream_t s, const IcpLattice* lat, const float4* q, int n, int* out_idx, float* out_d2) {
    if (n <= 0) return;
    const int g = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_lat_nn, dim3(g < 1024 ? g : 1024), dim3(BLOCK), 0, s, lat, q, n, out_idx, out_d2);
}

}  // namespace cd
