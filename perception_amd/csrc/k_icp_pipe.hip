// k_icp_pipe.hip - S6 ICP, pipelined whole-cluster driver: several clusters in flight per workgroup, no workgroup barrier inside the
// iteration loop (k_icp_pipe: template in LDS; k_icp_pipe_big: template in global memory), with the wave-per-query search of
// far queries over k-d patches, the slot protocol and the hand-over of running clusters between workgroups.
// This unit owns the ICP counters of the experiment builds (icp_debug.hpp): they cover k_icp_pipe / k_icp_pipe_big only.
#include "kernels.hpp"
#include "icp_solve.hpp"
#include "icp_debug.hpp"

namespace cd {
#if defined(CD_STATS) || defined(CD_TIMERS)
CD_DEBUG_COUNTERS(g_icp_stats, [16], cd_debug_icp_stats)
#endif
#ifdef CD_STATS
// far queries (seed ball wider than the grid walk's reach) by iteration class (0: it < 3, 1: it < 16, 2: later) and by the
// radius of the seed ball in grid cells (bucket 15: 15 or more)
CD_DEBUG_COUNTERS(g_icp_rhist, [48], cd_debug_icp_rhist)
#define CD_GRID_STAT(slot, cond) { const unsigned long long b_ = ballot64(cond); if ((threadIdx.x & 63) == 0) { atomicAdd(&g_icp_stats[slot], 1ull); atomicAdd(&g_icp_stats[(slot) + 1], (unsigned long long)__popcll(b_)); } }
// g_icp_stats[slot] += v, once per wave (v: wave-uniform, evaluated by every lane - it may hold a ballot)
#define CD_STAT_ADD(slot, v) { const unsigned long long v_ = (unsigned long long)(v); if ((threadIdx.x & 63) == 0) atomicAdd(&g_icp_stats[slot], v_); }
// [8] seed tests of a pass of nk queries in iteration `it`
#define CD_STAT_SEEDS(nk, it, m) CD_STAT_ADD(8, (unsigned long long)(nk) * (unsigned long long)(((it) > 0 ? 1 : 0) + ((it) < 3 ? ((m) + ICP_SUB - 1) / ICP_SUB : 0)))
// [0] queries, [3] near queries; the far ones of an iteration into the radius histogram
#define CD_STAT_NEAR(nk, near, mine_far, it, cells) { CD_STAT_ADD(0, nk) CD_STAT_ADD(3, __popcll(ballot64(near))) \
    if (mine_far) atomicAdd(&g_icp_rhist[((it) < 3 ? 0 : (it) < 16 ? 16 : 32) + min(15, (int)(cells))], 1ull); }
// far queries of an iteration ([12 + class]) and those whose TRUE neighbour lies within the grid walk's reach ([9 + class]: a
// better seed would have made them near), by iteration class
#define CD_STAT_REACH(mine_far, within, it) { const int cls_ = (it) < 3 ? 0 : (it) < 16 ? 1 : 2; \
    CD_STAT_ADD(9 + cls_, __popcll(ballot64((mine_far) && (within)))) CD_STAT_ADD(12 + cls_, __popcll(ballot64(mine_far))) }
#else
#define CD_STAT_ADD(slot, v)
#define CD_STAT_SEEDS(nk, it, m)
#define CD_STAT_NEAR(nk, near, mine_far, it, cells)
#define CD_STAT_REACH(mine_far, within, it)
#endif
#ifdef CD_ITSTATS
// per ICP iteration (31 = fitness pass): pass cycles, passes, far queries, patches visited
CD_DEBUG_COUNTERS(g_icp_it, [32][4], cd_debug_icp_it)
#define CD_IT_BEGIN(iter_phase, it) const long long tpass0_ = clock64(); const int stat_it_ = (iter_phase) ? min(it, 30) : 31; int stat_acc_[2] = {0, 0};
#define CD_IT_ACC stat_acc_
#define CD_IT_FAR(acc, npatches) if (acc) { (acc)[0] += 1; (acc)[1] += (npatches); }
#define CD_IT_END() if ((threadIdx.x & 63) == 0) { \
    atomicAdd(&g_icp_it[stat_it_][0], (unsigned long long)(clock64() - tpass0_)); atomicAdd(&g_icp_it[stat_it_][1], 1ull); \
    atomicAdd(&g_icp_it[stat_it_][2], (unsigned long long)stat_acc_[0]); atomicAdd(&g_icp_it[stat_it_][3], (unsigned long long)stat_acc_[1]); }
#else
#define CD_IT_BEGIN(iter_phase, it)
#define CD_IT_ACC nullptr
#define CD_IT_FAR(acc, npatches)
#define CD_IT_END()
#endif
#ifdef CD_TIMERS_FETCH
// how long a wave waits for its pass's points and neighbour indices (the loads that follow then hit L1): phase 3
#define CD_FETCH_WAIT(mine, p_pt, p_nn) { float4 pp_ = make_float4(0.f, 0.f, 0.f, 0.f); int nv_ = 0; if (mine) { pp_ = *(p_pt); nv_ = *(p_nn); } \
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(pp_.x), "v"(nv_) : "memory"); CD_PHASE(3) }
#else
#define CD_FETCH_WAIT(mine, p_pt, p_nn)
#endif
#ifdef CD_DONDBG
// hand-over timeline (tools/probe_handover.py): [1] latest workgroup end, [2] ticks spent waiting, [8 + b] waits begun,
// [24 + b] clusters published, [40 + b] clusters taken in quarter-millisecond bin b of the workgroup's own life (100 MHz ticks)
CD_DEBUG_COUNTERS(g_don_dbg, [64], cd_debug_don)
#endif
}  // namespace cd

#include "icp_search.hpp"

namespace cd {

// Wave-per-query search over k-d PATCHES of a cell-sorted template: patch r = the 64 stored positions s_kd[64 r ..], its box
// in bx.  The points stay where the grid walk wants them; this search gets the compact boxes it wants.  Lane l keeps the box
// of patch l of the LEFT half of the k-d root split and of patch l of the RIGHT half (psplit = patches in the left half);
// `need` says per query which halves its bound reaches at all (bit 0 / 1), so most queries test one box per lane, not two.
//
// Cost probes on the bench batch (the search run twice: +3.7 ms of 6.4; only the patch visits twice: +1.5 ms; only the box tests
// twice: +0.4 ms) showed where a far query's time goes: not into the arithmetic but into the control flow around it.  What
// paid: the lexicographic update as ONE 64-bit unsigned compare (the compiler turned "d < best || (d == best && oi < boi)"
// into two nested exec-mask regions with branches per patch), 6.4 -> 6.0 ms.  What did not: two queries interleaved per trip
// (same time: the SGPR pressure of two mask/coordinate sets spills to VGPR lanes).
struct FarQ { float x, y, z, best; unsigned long long m0, m1; unsigned long long lkey, seed; };   // lkey = d2 bits : (original index << 13 | stored position); seed: the query's seed key (wave-uniform)

// m with bit k cleared, in ONE scalar instruction (the compiler's m & (m - 1) is s_add_u32 + s_addc_u32 + s_and_b64).  The
// scalar unit is shared by the sixteen waves of the workgroup, and the far search issues 0.8 scalar instructions per vector
// instruction - three quarters of the kernel's scalar instructions (profiles/r04_valu_calibration.txt):
// every scalar instruction taken out of these loops is worth more than a vector one.
__device__ __forceinline__ unsigned long long clear_bit64(unsigned long long m, int k) {
    asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(k));
    return m;
}

// The query enters with ITS SEED'S KEY (round 4): q.pbest = d2(q, seed) exactly, q.poi = the seed's key word.  The box
// test `lb <= d2(q, seed)` keeps every patch that can hold a point as close as the seed (closer, or equally close with a lower
// original index); the lanes' running minima start at the seed key, so "some lane's key is below the seed key" says exactly
// "the neighbour changes" - and when it does not (the usual case once ICP has settled) the query is done after the visits:
// no reduction, no write-back.  far_query broadcasts query k of the wave and its seed key; both far searches start with it.
__device__ __forceinline__ void far_query(FarQ& f, const QueryRegs& q, int k) {
    f.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.px), k));
    f.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.py), k));
    f.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.pz), k));
    f.best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.pbest), k));
    f.lkey = ((unsigned long long)__float_as_uint(f.best) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readlane(q.poi, k);
    f.seed = f.lkey;
}
__device__ __forceinline__ void far_take(FarQ& f, const float4& t) {
    // lexicographic (d2, original index) minimum, rule C5, as ONE unsigned 64-bit compare: squared distances are non-negative
    // floats (or +inf / NaN-free here), which order like their bit patterns; no branch, no tie special case
    // The low word carries the stored position below the original index (both < 2^13 for an LDS-resident template; the
    // position is a function of the index, so the order is still (d2, original index)): the key alone is the whole answer.
    const float d = dist2(f.x, f.y, f.z, t.x, t.y, t.w);   // (the re-labelled image: (x, y, key word, z), see tpl_z)
    unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(t.z);
    asm("" : "+v"(key));   // (as in grid_search: keeps the key in the loaded quad's own registers)
    f.lkey = key < f.lkey ? key : f.lkey;
}
// Minimum over the wave WITHOUT a reduction: the query's owner lane puts the bound key into the wave's LDS word, every lane
// that beat the bound takes an LDS 64-bit atomic min on it (same address: the LDS serialises them, one per clock), and the
// word is read back - by all lanes, broadcast - and unpacked.  LDS operations of one wave execute in program order, so no
// fence is needed.  This replaced ballot + popcount + (DPP minimum + tie loop | three v_readlane) + a masked write-back,
// which cost more than the box tests (probe: the tail run twice = +1.05 ms of 5.9).
template <unsigned POS_MASK>
__device__ __forceinline__ void far_merge(unsigned long long lkey, unsigned long long bound, QueryRegs& q, int k, unsigned long long* slot) {
    const int lane = threadIdx.x & 63;
    // lanes whose key beats the seed's.  None (the usual case once ICP has settled: the neighbour is still the seed): the
    // query keeps it, nothing to do.  Exactly one: that key IS the minimum, fetched with two readlanes.  Several: LDS 64-bit
    // min over them.
    const unsigned long long imp = ballot64(lkey < bound);
    if (imp == 0ull) return;
    unsigned long long res;
    if (__popcll(imp) == 1) {
        const int src = __ffsll((long long)imp) - 1;
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(lkey >> 32), src);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)lkey, src);
        res = ((unsigned long long)hi << 32) | lo;
    } else {
        if (lane == k) __hip_atomic_store(slot, bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (lkey < bound) __hip_atomic_fetch_min(slot, lkey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        res = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    const bool mine = lane == k;
    const unsigned lo = (unsigned)res;
    q.pbest = mine ? __uint_as_float((unsigned)(res >> 32)) : q.pbest;
    q.pbi = mine ? (int)(lo & POS_MASK) : q.pbi;
    q.poi = mine ? (int)lo : q.poi;
}
__device__ __forceinline__ void search_patches(const float4* s_tpl, const unsigned short* s_kd, const RunBoxes& bx, QueryRegs& q,
                                               unsigned long long todo, int psplit, unsigned long long* slot, int* stat_acc = nullptr) {
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int k = __ffsll((long long)todo) - 1;
        todo = clear_bit64(todo, k);
        FarQ A;
        far_query(A, q, k);
        // Both halves' boxes are always tested: the per-query flag that skipped an unreachable half cost a readlane, two scalar
        // bit tests and two branches to save eleven vector instructions - on a scalar unit that sixteen waves share.
        A.m0 = ballot64(box_lb(bx.L0, bx.H0, A.x, A.y, A.z) <= A.best);
        A.m1 = ballot64(box_lb(bx.L1, bx.H1, A.x, A.y, A.z) <= A.best);
        CD_STAT_ADD(1, __popcll(A.m0) + __popcll(A.m1)) CD_STAT_ADD(2, 1)   // [2] far queries searched, [1] the patches they visit
        CD_IT_FAR(stat_acc, __popcll(A.m0) + __popcll(A.m1))
        // the two halves' masks one after the other: no per-patch choice between them (three scalar instructions and a branch)
        while (A.m0) {
            const int r = __ffsll((long long)A.m0) - 1;
            A.m0 = clear_bit64(A.m0, r);
            const int pos = s_kd[r * ICP_SUB + lane];
            far_take(A, s_tpl[pos]);
        }
        const unsigned short* s_kd1 = s_kd + psplit * ICP_SUB;   // (the right half's table: no per-patch scalar add)
        while (A.m1) {
            const int r = __ffsll((long long)A.m1) - 1;
            A.m1 = clear_bit64(A.m1, r);
            const int pos = s_kd1[r * ICP_SUB + lane];
            far_take(A, s_tpl[pos]);
        }
        far_merge<KeyFmt<13>::POS_MASK>(A.lkey, A.seed, q, k, slot);
    }
}


// ---------------------------------------------------------------------------------------
// Wave-per-query search over a template that does NOT fit LDS (more than ICP_TPL_LDS points; up to 65535): the points stay in
// global memory (a few hundred KiB: L2-resident) in k-d patch order, so a patch is ONE coalesced 1 KiB read; the patch boxes
// (32 B each) are in LDS, and a second level above them - the boxes of k-d subtrees of at most 64 patches ("superpatches",
// IcpSuper; lane l keeps superpatch l's box in registers) - tells with one ballot which runs of <= 64 patch boxes need
// testing at all.  Same exactness argument as the run boxes: a box bound is a lower bound of the canonical float distance
// to everything inside it, and a superpatch box contains its patch boxes.
// ---------------------------------------------------------------------------------------
struct SuperRegs { float4 L, H; int first, cnt; };   // lane l: box, first patch and patch count of superpatch l (+inf box: none)

__device__ __forceinline__ void search_patches_big(const float4* __restrict__ tplk, const unsigned short* __restrict__ kdmap,
                                                   const float4* s_plo, const float4* s_phi, const SuperRegs& sp, QueryRegs& q,
                                                   unsigned long long todo, unsigned long long* slot) {
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int k = __ffsll((long long)todo) - 1;
        todo = clear_bit64(todo, k);
        FarQ A;   // (m0, m1 unused: the boxes here are the superpatches')
        far_query(A, q, k);
        unsigned long long ma = ballot64(box_lb(sp.L, sp.H, A.x, A.y, A.z) <= A.best);
        CD_STAT_ADD(2, 1)
        while (ma) {
            const int sidx = __ffsll((long long)ma) - 1;
            ma = clear_bit64(ma, sidx);
            const int first = __builtin_amdgcn_readlane(sp.first, sidx), cnt = __builtin_amdgcn_readlane(sp.cnt, sidx);
            const int pl = first + min(lane, cnt - 1);
            unsigned long long mp = ballot64(lane < cnt && box_lb(s_plo[pl], s_phi[pl], A.x, A.y, A.z) <= A.best);
            CD_STAT_ADD(1, __popcll(mp))
            while (mp) {   // two patches per trip: their loads are in flight together (an odd one out is read twice)
                const int b0 = __ffsll((long long)mp) - 1;
                mp = clear_bit64(mp, b0);
                const int b1 = mp ? __ffsll((long long)mp) - 1 : b0;
                mp = clear_bit64(mp, b1);          // (clearing a bit that is already clear changes nothing)
                const int r0 = first + b0, r1 = first + b1;
                const float4 t = tplk[(unsigned)(r0 * ICP_SUB + lane)];
                const float4 u = tplk[(unsigned)(r1 * ICP_SUB + lane)];
                const unsigned pt = kdmap[(unsigned)(r0 * ICP_SUB + lane)];
                const unsigned pu = kdmap[(unsigned)(r1 * ICP_SUB + lane)];
                const float d = dist2(A.x, A.y, A.z, t.x, t.y, t.z);
                const float e = dist2(A.x, A.y, A.z, u.x, u.y, u.z);
                const unsigned long long kd_ = ((unsigned long long)__float_as_uint(d) << 32) | (((unsigned)__float_as_int(t.w) << 16) | pt);
                const unsigned long long ke_ = ((unsigned long long)__float_as_uint(e) << 32) | (((unsigned)__float_as_int(u.w) << 16) | pu);
                A.lkey = kd_ < A.lkey ? kd_ : A.lkey;
                A.lkey = ke_ < A.lkey ? ke_ : A.lkey;
            }
        }
        far_merge<KeyFmt<16>::POS_MASK>(A.lkey, A.seed, q, k, slot);
    }
}

// ---------------------------------------------------------------------------------------
// k_icp_pipe: whole-cluster ICP with TWO clusters in flight per workgroup and no workgroup
// barrier inside the iteration loop.
//
// k_icp_cluster spends about a fifth of its time in the per-iteration barrier (waves of one
// workgroup finish their share of an iteration at different times) and another tenth in the
// single-threaded Umeyama/SVD solve that 1023 threads wait for.  Here a workgroup owns up to
// CD_PIPE_SLOTS cluster slots (same template in LDS; the launch says how many it uses: two when it
// has the GPU to itself, four when the GPU is shared).  Every wave walks the slots round-robin:
//   wait until the slot's epoch says the previous step has been solved  ->  do its own share of
//   the slot's current step (a fixed set of source points per lane, as in k_icp_cluster)  ->
//   add its 16 fixed-point moment sums to the slot's LDS accumulators  ->  count itself arrived.
// The wave that arrives LAST runs the solve for that step (or the fitness hand-over and the
// refill of the slot from the global cluster queue) and bumps the epoch, while the other
// fifteen waves are already working on the other slots.  All waves visit the same sequence of
// (slot, epoch) steps and the slowest wave never waits for anything but a solve in progress, so
// there is no circular wait; a slot whose queue ran dry is published as exhausted through the
// same epoch mechanism and every wave leaves after seeing every slot exhausted.
// Arithmetic is that of k_icp_cluster / k_icp_iter + k_icp_solve + k_icp_fitness (order-free
// integer moment sums), so results are bit-identical.
// ---------------------------------------------------------------------------------------
constexpr int PIPE_SLOTS = CD_PIPE_SLOTS;   // most clusters in flight per workgroup (common.hpp); the launch says how many it uses
static_assert(PIPE_SLOTS >= 1 && PIPE_SLOTS <= 8, "one byte of the packed per-wave step counters per slot");   // (common.hpp allows 6: LDS)
enum { PH_ITER = 0, PH_FIT = 1, PH_EXHAUSTED = 2, PH_FILL = 3 };

struct PipeSlot {
    IcpState so;                    // T = transformation_ of the current iteration, Tfinal = accumulated
    unsigned long long acc[16];     // moment sums of the current step
    int src_off, n, k;              // the cluster
    int phase, it;
    int arrived;                    // waves that finished their share of the current step
    int epoch;                      // steps completed (solved) so far
    int next_pass;                  // next 64-point pass of the current step nobody has taken yet
    int give;                       // 1: the cluster is promised to a waiting workgroup - this step's stores of its points and neighbour indices go
                                    // through to memory (agent scope), then it leaves
    int take;                       // 1: the cluster has just arrived from another workgroup - this step reads them past L1 / L2 (agent scope)
};
// the slot of the BOUNDED instantiations (rule C8): + the kept correspondences of the current step, an order-free count next to
// the moment sums (zeroed with them; a hand-over happens between steps, so like them it never travels).  The default layout -
// and so the LDS budget of common.hpp - stays as it is.
struct PipeSlotN : PipeSlot {
    uint32_t nv, pad;
};
template <bool BOUNDED> struct PipeSlotSel { using T = PipeSlot; };
template <> struct PipeSlotSel<true> { using T = PipeSlotN; };

// A slot ready for the passes and arrivals of a step: sums (and kept count) zero, nobody arrived, no pass taken
template <bool BOUNDED, class Slot>
__device__ __forceinline__ void pipe_slot_clear(Slot* sl) {
    for (int i = 0; i < 16; ++i) sl->acc[i] = 0ull;
    if constexpr (BOUNDED) sl->nv = 0u;
    sl->arrived = 0;
    sl->next_pass = 0;
}

// The state update of one iteration (icp_step; lane 0 of the finishing wave).  BOUNDED (rule C8): n = the kept correspondences.
// (Out-of-line callees are plain overloads, not template instances: a linkonce function has no exact definition,
// so its callers could not use its register usage - k_icp_pipe would allocate more registers around the call.)
__device__ __noinline__ int pipe_solve(PipeSlot* sl, const IcpParams& prm) { return icp_step<false>(sl->so, sl->acc, sl->n, prm); }
__device__ __noinline__ int pipe_solve(PipeSlotN* sl, const IcpParams& prm) { return icp_step<true>(sl->so, sl->acc, (int)sl->nv, prm); }

// next cluster from the global queue into the slot (lane 0 of the finishing wave)
// (items [gbeg, gend) of `order`: the clusters that share the workgroup's template)
__device__ __forceinline__ void pipe_refill(PipeSlot* sl, int gbeg, int gend, const int* order, const IcpCluster* cl, const IcpState* st, int* queue,
                                            int* don, bool no_queue = false) {
    sl->give = 0; sl->take = 0;
    if (no_queue) { sl->phase = PH_EXHAUSTED; return; }   // (IcpParams::don_idle: this workgroup only ever works on hand-overs)
    for (;;) {
        const int item = gbeg + atomicAdd(queue, 1);
        if (item >= gend) { sl->phase = PH_EXHAUSTED; return; }
        const int k = order[item];
        if (st[2 * (size_t)k].done) {                    // host pre-marked (too few points / no template)
            if (don) __hip_atomic_fetch_add(don + DON_FINISHED, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const IcpCluster c = cl[k];
        sl->src_off = c.src_off; sl->n = c.n; sl->k = k;
        sl->so = st[2 * (size_t)k];
        sl->phase = PH_ITER; sl->it = 0;
        return;
    }
}

// ---- hand-over of running clusters (IcpParams::donate; launches that have the GPU to themselves) ---------------------------
// The bench batch is 522 clusters on 256 workgroups: two each, of 6 to 100 iterations that nothing predicts - the slowest
// workgroup runs 4.4 ms, the average one 3.5 (tools/probe_balance.py).  A workgroup that finds the queue empty with nothing
// left of its own therefore WAITS (one lane polls, the others sit at a barrier) instead of ending, and a workgroup that still
// has two or more clusters going gives one of them away:
//   waiter : DON_AVAIL += 1, then polls the mailbox (and DON_FINISHED == clusters of the launch -> ends)
//   donor  : at a step boundary sees DON_AVAIL > 0, takes one (DON_AVAIL -= 1: one promise per waiter) and sets the slot's `give`;
//            during the NEXT step every wave writes the cluster's points and neighbour indices with agent-scope (sc1) stores -
//            through to memory: the taker may sit on another XCD, whose L2 is not coherent with this one - and waits for them
//            (vmcnt) before it arrives; at the end of that step the finishing wave writes the slot's IcpState to st[] the same
//            way, waits, and publishes the cluster id in the next mailbox entry.  (A cluster that converged in that very step
//            is not handed over: the promise is returned, DON_AVAIL += 1.)
//   taker  : reads the entry and the state with agent-scope loads, sets the slot's `take`: in the cluster's FIRST step here every
//            wave reads its points and indices with agent-scope loads (past this CU's L1 and this XCD's L2, which may hold
//            lines from an earlier stay of the cluster); that step rewrites every point and index, so plain accesses are right
//            again from the second step on.  The arithmetic does not depend on who executes it: the records are bit-identical
//            with or without hand-overs (tests/test_gpu_timed_path.py).
// (First version: agent-scope FENCES - every wave of the give step wrote back its XCD's whole L2, the taker invalidated its own.
//  Same time, but the launch's HBM traffic went from 0.26 to 0.48 GB; profiles/r04_handover.txt.)
// Nobody ever waits for a donor or a taker: donors never block, and a waiter's poll ends when every cluster is finished,
// which the running workgroups reach on their own.  Both polls carry a bound all the same.
__device__ __forceinline__ int don_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// agent-scope (sc1) accesses of a cluster's points and neighbour indices: written through to memory / read past this CU's L1
// and this XCD's L2, dword by dword (relaxed atomics: the orderings come from s_waitcnt and the mailbox entry)
__device__ __forceinline__ void store_agent(float4* p, const float4& v) {
    unsigned* u = reinterpret_cast<unsigned*>(p);
    __hip_atomic_store(u + 0, __float_as_uint(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(u + 1, __float_as_uint(v.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(u + 2, __float_as_uint(v.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(u + 3, __float_as_uint(v.w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float4 load_agent(const float4* p) {
    const unsigned* u = reinterpret_cast<const unsigned*>(p);
    const unsigned x = __hip_atomic_load(u + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), y = __hip_atomic_load(u + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned z = __hip_atomic_load(u + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), w = __hip_atomic_load(u + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float4(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z), __uint_as_float(w));
}
// the slot's IcpState to / from st[] the same way (lane 0; 40 dwords)
__device__ __forceinline__ void state_store_agent(IcpState* dst, const IcpState& src) {
    static_assert(sizeof(IcpState) % 4 == 0, "IcpState is copied dword by dword");
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    const unsigned* s = reinterpret_cast<const unsigned*>(&src);
    for (int i = 0; i < (int)(sizeof(IcpState) / 4); ++i) __hip_atomic_store(d + i, s[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void state_load_agent(IcpState& dst, const IcpState* src) {
    unsigned* d = reinterpret_cast<unsigned*>(&dst);
    const unsigned* s = reinterpret_cast<const unsigned*>(src);
    for (int i = 0; i < (int)(sizeof(IcpState) / 4); ++i) d[i] = __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class Slot>
__device__ __forceinline__ int pipe_active_slots(const Slot* slots) {
    int a = 0;
    for (int i = 0; i < PIPE_SLOTS; ++i) a += (slots[i].phase == PH_ITER || slots[i].phase == PH_FIT) ? 1 : 0;
    return a;
}
// lane 0 of the finishing wave, cluster not converged: returns true when the slot's cluster went to the mailbox
template <class Slot>
__device__ __forceinline__ bool pipe_give_body(Slot* sl, const Slot* slots, IcpState* st, int* don, bool fault) {
    bool gone = false;
    if (pipe_active_slots(slots) >= 2) {
        state_store_agent(&st[2 * (size_t)sl->k], sl->so);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the state is in memory before the entry says so
        const int t = __hip_atomic_fetch_add(don + DON_TAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t < DON_CAP) {
            if (!(fault && t == 0))   // (fault injection, tests: the first entry is claimed and never written)
                __hip_atomic_store(don + DON_BOX + t, sl->k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gone = true;
        }
    }
    if (!gone) __hip_atomic_fetch_add(don + DON_AVAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // promise returned
    sl->give = 0;
    return gone;
}
__device__ __noinline__ bool pipe_give(PipeSlot* sl, const PipeSlot* slots, IcpState* st, int* don, bool fault) {
    return pipe_give_body(sl, slots, st, don, fault);
}
__device__ __noinline__ bool pipe_give(PipeSlotN* sl, const PipeSlotN* slots, IcpState* st, int* don, bool fault) {
    return pipe_give_body(sl, slots, st, don, fault);
}
// thread 0 of a workgroup with nothing left: the id of a cluster to carry on with, or -1 when the launch is finished
// Both bail-outs are REPORTED (DON_ERR; the host fails the call with CD_ERR_DEVICE): an entry that was claimed and never
// appeared means its cluster left its donor and reached nobody; running out of polls with clusters still open means the
// launch's bookkeeping is off.  Neither can happen in a healthy launch (a donor stores the entry right after claiming its
// index; every running workgroup finishes its clusters on its own) - tests/test_gpu_timed_path.py injects the first.
__device__ __noinline__ int pipe_wait_for_cluster(int* don, int total, int entry_spins) {
    __hip_atomic_fetch_add(don + DON_AVAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int polls = 0; polls < (1 << 22); ++polls) {
        const int head = don_load(don + DON_HEAD), tail = min(don_load(don + DON_TAIL), DON_CAP);
        if (head < tail) {
            int expect = head;
            if (__hip_atomic_compare_exchange_strong(don + DON_HEAD, &expect, head + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                int v = 0;
                for (int spins = 0; spins < entry_spins && v == 0; ++spins) v = don_load(don + DON_BOX + head);
                if (v == 0) __hip_atomic_store(don + DON_ERR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // claimed, never published
                return v - 1;
            }
            continue;
        }
        if (don_load(don + DON_FINISHED) >= total) return -1;
        if (don_load(don + DON_ERR)) return -1;   // (somebody lost a cluster: FINISHED will never reach the total)
        __builtin_amdgcn_s_sleep(32);
    }
    __hip_atomic_fetch_add(don + DON_AVAIL, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // this waiter is gone: no donor may promise it a cluster
    __hip_atomic_store(don + DON_ERR, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return -1;
}

// A template point as icp_pipe_body reads it.  BIG: (x, y, z, original index) from global memory, the key word put together
// from the index and the stored position.  Otherwise the LDS image, re-labelled once at staging: the low word of a search key,
// (original index << 13) | position (pads: all ones, and +inf coordinates anyway), replaces the bare original index, which
// nothing in this kernel needs, and the point is stored as (x, y, key word, z): the key word then sits in the even register
// of the loaded quad and the squared distance can be formed in the z register next to it - the 64-bit key (rule C5's compare)
// needs no move
template <bool BIG> __device__ __forceinline__ float tpl_z(const float4& t) { return BIG ? t.z : t.w; }
template <bool BIG> __device__ __forceinline__ unsigned tpl_key_word(const float4& t, int pos) {
    return BIG ? (((unsigned)__float_as_int(t.w) << 16) | (unsigned)pos) : (unsigned)__float_as_int(t.z);
}

// A seed candidate of the query (x, y, z): the template point at `pos`, its squared distance and its key word.  The pass picks
// among them as icp_search.hpp's seed_query does, but remembers the seed's key word, which both searches start from.
struct PipeSeed { float d2; int pos; unsigned kw; };
template <bool BIG>
__device__ __forceinline__ PipeSeed seed_at(const float4* tpl, int pos, float x, float y, float z) {
    const float4 t = BIG ? tpl[(unsigned)pos] : tpl[pos];
    return {dist2(x, y, z, t.x, t.y, tpl_z<BIG>(t)), pos, tpl_key_word<BIG>(t, pos)};
}

// The pass's correspondences into the slot.  Iteration: the neighbour's index to *nnp (through to memory if the cluster leaves
// after this step) and the 16 moment terms of the kept ones, counted in nv if BOUNDED; fitness pass: the squared distance.  They go
// into the slot's accumulators right away: no sum is carried in registers across the searches (32 VGPRs that they would spill).
template <bool BIG, bool BOUNDED, class Slot>
__device__ __forceinline__ void pipe_fold_pass(Slot* sl, const float4* tpl, const QueryRegs q, int nk, int phase, int give, int* nnp, float d2_max) {
    const int lane = threadIdx.x & 63;
    unsigned long long S[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0ull;
    // float -> fixed point (rule C4) in four instructions per term instead of eight (fixq_fast, common.hpp), valid
    // while every term stays below 2^50 / 2^shift; a wave with a lane outside that range (coordinates beyond 256 m,
    // neighbours more than 128 m away) takes the general conversion - same integers either way
    float4 qq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < nk && phase == PH_ITER) qq = BIG ? tpl[(unsigned)q.pbi] : tpl[q.pbi];
    const float pv[3] = {q.px, q.py, q.pz}, qv[3] = {qq.x, qq.y, tpl_z<BIG>(qq)};
    const float big_c = fmaxf(fmaxf(fmaxf(fabsf(pv[0]), fabsf(pv[1])), fabsf(pv[2])), fmaxf(fmaxf(fabsf(qv[0]), fabsf(qv[1])), fabsf(qv[2])));
    const bool fast = ballot64(lane < nk && !(big_c < 256.f && q.pbest < 16384.f)) == 0ull;
    if (lane < nk) {
        if (phase == PH_ITER) {
            if (give) __hip_atomic_store(nnp, q.pbi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else *nnp = q.pbi;
            if (BOUNDED && !(q.pbest <= d2_max)) {
                // rejected (rule C8): adds nothing
            } else if (fast) {
                moment_terms<true>(pv, qv, q.pbest, S);
            } else {
                moment_terms(pv, qv, q.pbest, S);
            }
        } else {
            S[0] = fast ? fixq_fast(q.pbest, FIX_SHIFT_D2) : (unsigned long long)fixq(q.pbest, FIX_SHIFT_D2);
        }
    }
    wave_fold_to_lds(S, phase == PH_ITER ? 16 : 1, sl->acc);
    if constexpr (BOUNDED) {
        const unsigned long long kb = ballot64(lane < nk && phase == PH_ITER && q.pbest <= d2_max);
        if (lane == 0 && kb) atomicAdd(&sl->nv, (uint32_t)__popcll(kb));
    }
}

// Lane 0 of the wave that arrived last, end of an iteration: the state update; then a cluster that has not converged and was
// promised leaves for the mailbox (returns true: the slot is free), or is promised now if workgroups wait and this one has two
template <class Slot>
__device__ __forceinline__ bool pipe_end_iteration(Slot* sl, const Slot* slots, IcpState* st, int* don, const IcpParams& prm) {
    // (the load is in flight while the step is solved)
    const int waiting = don ? don_load(don + DON_AVAIL) : 0;
    sl->take = 0;
    if (pipe_solve(sl, prm)) {
        sl->phase = PH_FIT;
        if (sl->give) { sl->give = 0; __hip_atomic_fetch_add(don + DON_AVAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // converged: stays
        return false;
    }
    sl->it += 1;
    if (sl->give) return pipe_give(sl, slots, st, don, prm.don_fault != 0);
    if (waiting > 0 && pipe_active_slots(slots) >= 2) {
        // promise this cluster to one of the waiting workgroups; it goes after the next step
        if (__hip_atomic_fetch_add(don + DON_AVAIL, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) sl->give = 1;
        else __hip_atomic_fetch_add(don + DON_AVAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return false;
}
// thread 0, after pipe_wait_for_cluster: cluster k, handed over by another workgroup, carries on in slot sl
template <bool BOUNDED, class Slot>
__device__ __forceinline__ void pipe_take_over(Slot* sl, int k, const IcpCluster* __restrict__ cl, const IcpState* st) {
    const IcpCluster c = cl[k];
    sl->src_off = c.src_off; sl->n = c.n; sl->k = k;
    state_load_agent(sl->so, &st[2 * (size_t)k]);
    sl->phase = PH_ITER; sl->it = sl->so.iters; sl->give = 0; sl->take = 1;
    pipe_slot_clear<BOUNDED>(sl);
}

// BIG = false: k_icp_pipe, the template (<= ICP_TPL_LDS points) and its k-d position table live in LDS.
// BIG = true : k_icp_pipe_big, a template of up to 65535 points stays in global memory (L2-resident: a few hundred KiB read by
//              every workgroup) - the grid walk reads the cell-sorted copy `tpl` point by point, the wave-per-query search the
//              k-d ordered copy `tplk` patch by patch (search_patches_big); LDS holds the cell start table and the patch boxes.
//              Same pipeline, same arithmetic, same tie rule: bit-identical results (keys carry 16-bit positions).
// BOUNDED (rule C8): only correspondences with d2 <= bnd.d2_max enter the sums; the slot's nv counts them.
template <bool BIG, bool BOUNDED>
__device__ __forceinline__ void icp_pipe_body(int ncl, const int* __restrict__ order,
                                              const IcpCluster* __restrict__ cl, IcpState* st,
                                              unsigned long long* __restrict__ accf,
                                              const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                              const float4* __restrict__ thi,
                                              const unsigned short* __restrict__ kdmap,
                                              const IcpGrid* __restrict__ grids,
                                              const unsigned short* __restrict__ tcell, float4* src,
                                              const float4* __restrict__ src0, int* nn, int* queue,
                                              const int* __restrict__ wgtab, IcpParams prm,
                                              const float4* __restrict__ tplk, const IcpSuper* __restrict__ supers, const IcpBound& bnd) {
    __shared__ float4 s_tpl[BIG ? 1 : ICPT_IMG];
    __shared__ unsigned short s_cs[ICP_MAX_CELLS + 8];
    using Slot = typename PipeSlotSel<BOUNDED>::T;
    __shared__ Slot s_slot[PIPE_SLOTS];
    __shared__ unsigned short s_kd[BIG ? 1 : ICPT_IMG];   // k-d patch order -> stored position (tlo/thi are the PATCH boxes)
    __shared__ unsigned long long s_far[ICPT_WAVES];   // one word per wave: the running minimum of the far query it is on
    __shared__ float4 s_plo[BIG ? ICP_BIG_PATCHES : 1], s_phi[BIG ? ICP_BIG_PATCHES : 1];   // BIG: boxes of all k-d patches
    constexpr int KSH = BIG ? 16 : 13;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // A workgroup keeps ONE (LDS-resident, gridded) template for its whole life.  With several templates in a launch
    // (every cluster against every template, opd flavour with template_slot = -1) the host groups the clusters by template,
    // gives every group a share of the workgroups and its own queue: wgtab[3 b] = {first item, end item, queue} of
    // workgroup b; without a table all clusters share one template and one queue.
    int gbeg = 0, gend = ncl;
    if (wgtab) { gbeg = wgtab[3 * blockIdx.x]; gend = wgtab[3 * blockIdx.x + 1]; queue += wgtab[3 * blockIdx.x + 2]; }
    int* const don = (prm.donate && !wgtab) ? prm.don : nullptr;   // (hand-overs: launches with one queue only)
    const bool no_queue = don && (int)blockIdx.x < prm.don_idle;   // (tests: this workgroup only ever gets work by hand-over)
    __shared__ int s_take;
    const IcpCluster c0 = cl[order[gbeg]];
    const IcpGrid g = grids[c0.slot];
    const float4* tp = tpl + c0.tpl_off;
    const int tpl_m = c0.tpl_m;
    const float rmax = __fmul_rn(prm.grid_rc, g.cell);
    // the point a lane without work reads: the first point of the +inf pad run of the staged image; from global memory the
    // template's last point (testing a real template point is always harmless: it can only be the answer if it is the answer)
    const int gpad = BIG ? tpl_m - 1 : (tpl_m + ICP_SUB - 1) / ICP_SUB * ICP_SUB;
    RunBoxes bx;
    SuperRegs sp;
    const float4* tk = BIG ? tplk + c0.tpl_off : nullptr;
    const unsigned short* km = kdmap + c0.tpl_off;
    for (int i = threadIdx.x; i <= g.ncell; i += ICPT_THREADS) s_cs[i] = tcell[g.cell_off + i];
    if constexpr (!BIG) {
        for (int i = threadIdx.x; i < (tpl_m + ICP_SUB - 1) / ICP_SUB * ICP_SUB; i += ICPT_THREADS) s_kd[i] = km[i];
        stage_chunk(tp, tlo + c0.tpl_off / ICP_SUB, thi + c0.tpl_off / ICP_SUB, 0, tpl_m, s_tpl, bx);
        // re-label the image as (x, y, key word, z): see tpl_z
        for (int i = threadIdx.x; i < (tpl_m + ICP_SUB - 1) / ICP_SUB * ICP_SUB + ICP_SUB; i += ICPT_THREADS) {
            const float4 p = s_tpl[i];
            const unsigned oi = (unsigned)__float_as_int(p.w);
            s_tpl[i] = make_float4(p.x, p.y, __uint_as_float(i < tpl_m ? ((oi << 13) | (unsigned)i) : 0xffffffffu), p.z);
        }
        __syncthreads();
    } else {
        const int nruns = (tpl_m + ICP_SUB - 1) / ICP_SUB;
        for (int i = threadIdx.x; i < nruns; i += ICPT_THREADS) { s_plo[i] = tlo[c0.tpl_off / ICP_SUB + i]; s_phi[i] = thi[c0.tpl_off / ICP_SUB + i]; }
        const IcpSuper& su = supers[c0.slot];
        const float inf = __uint_as_float(0x7f800000u);
        sp.L = sp.H = make_float4(inf, inf, inf, 0.f);
        sp.first = 0; sp.cnt = 1;
        if (lane < su.n) {
            sp.L = make_float4(su.lo[lane][0], su.lo[lane][1], su.lo[lane][2], 0.f);
            sp.H = make_float4(su.hi[lane][0], su.hi[lane][1], su.hi[lane][2], 0.f);
            sp.first = su.first[lane]; sp.cnt = su.cnt[lane];
        }
        __syncthreads();
    }
    // lane l keeps the boxes of patch l of the LEFT half of the k-d root split and of patch l of the RIGHT half
    const int psplit = g.kd_split;
    if constexpr (!BIG) {
        const int nruns = (tpl_m + ICP_SUB - 1) / ICP_SUB;
        const float inf = __uint_as_float(0x7f800000u);
        const float4 none = make_float4(inf, inf, inf, 0.f);
        const float4* blo = tlo + c0.tpl_off / ICP_SUB;
        const float4* bhi = thi + c0.tpl_off / ICP_SUB;
        bx.L0 = bx.H0 = bx.L1 = bx.H1 = none;
        if (lane < psplit) { bx.L0 = blo[lane]; bx.H0 = bhi[lane]; }
        if (psplit + lane < nruns) { bx.L1 = blo[psplit + lane]; bx.H1 = bhi[psplit + lane]; }
    }
    if (threadIdx.x == 0) {
        for (int sidx = 0; sidx < PIPE_SLOTS; ++sidx) {
            Slot* sl = &s_slot[sidx];
            pipe_slot_clear<BOUNDED>(sl);
            sl->epoch = 0; sl->it = 0; sl->n = 0; sl->src_off = 0; sl->k = 0; sl->give = 0; sl->take = 0;
            sl->phase = sidx < prm.pipe_slots ? PH_FILL : PH_EXHAUSTED;   // (a slot the launch does not use is dropped at its first visit)
        }
        // slot 0 starts with a cluster; the other slots are filled at their first step (PH_FILL), after every workgroup took its first
        pipe_refill(&s_slot[0], gbeg, gend, order, cl, st, queue, don, no_queue);
        if (no_queue) for (int sidx = 0; sidx < PIPE_SLOTS; ++sidx) s_slot[sidx].phase = PH_EXHAUSTED;
    }
    __syncthreads();
    CD_TIMERS_BEGIN
    DON_DBG_BEGIN
    // per wave: the steps it has completed on each slot (one byte per slot, mod 256: waves are never a whole step apart) and
    // the slots that still have work
    unsigned long long my_ep = 0ull;
    unsigned live = (1u << PIPE_SLOTS) - 1u;
    for (;;) {
    while (live) {
        for (int sidx = 0; sidx < PIPE_SLOTS; ++sidx) {
            if (!((live >> sidx) & 1u)) continue;
            Slot* sl = &s_slot[sidx];
            // wait for the slot's epoch: the previous step has been finished
            const int want = (int)((my_ep >> (8 * sidx)) & 0xffu);
            while (__hip_atomic_load(&sl->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != want) __builtin_amdgcn_s_sleep(2);
            __threadfence_block();
            CD_PHASE(0)
            const int phase = sl->phase;
            if (phase == PH_EXHAUSTED) { live &= ~(1u << sidx); continue; }
            const int give = sl->give;   // the cluster leaves this workgroup after this step: its stores must reach memory
            const int take = sl->take;   // it arrived before this step: its points and indices are read from memory
            if (phase == PH_ITER || phase == PH_FIT) {
                const int it = sl->it, n = sl->n;
                float4* pts = src + sl->src_off;
                const float4* pts0 = src0 + sl->src_off;
                int* nnq = nn + sl->src_off;
                // The step's queries are cut into passes of 64 consecutive points; waves PULL passes from the slot's
                // counter, so a wave that drew cheap passes (certainly-near queries) simply takes more of them and all
                // waves reach the end of the step together.  (A point is then touched by different waves in different
                // steps: same CU, and the step boundary is a workgroup-scope release/acquire.)
                const int npass = (n + 63) >> 6;
                for (;;) {   // this wave's share of the step, pass by pass
                    int pss = 0;
                    if (lane == 0) pss = atomicAdd(&sl->next_pass, 1);
                    pss = __builtin_amdgcn_readfirstlane(pss);
                    if (pss >= npass) break;
                    const int q0 = pss << 6;
                    const int nk = min(64, n - q0);
                    const int myq = q0 + lane;
                    CD_IT_BEGIN(phase == PH_ITER, it)
                    QueryRegs q;
                    q.px = q.py = q.pz = q.pbest = 0.f; q.pbi = 0; q.poi = 0x7fffffff;
                    // key word of the seed point: what the LDS image holds in .z, (original index << 16) | position for a
                    // template in global memory; "no index" while there is no seed
                    unsigned kw = KeyFmt<KSH>::NONE;
                    CD_FETCH_WAIT(lane < nk, &pts[myq], &nnq[myq])
                    // fetch the pass's queries and seed them (as functions this costs the pass loop instructions: profiles/EXPERIMENTS.md)
                    if (lane < nk) {
                        const float4 p = take ? load_agent(&pts[myq]) : pts[myq];
                        if (phase == PH_ITER) {
                            q.px = p.x; q.py = p.y; q.pz = p.z;
                            if (it > 0) {   // X <- T*X, written back by the lane that owns the point
                                xform(sl->so.T, p.x, p.y, p.z, q.px, q.py, q.pz);
                                if (give) store_agent(&pts[myq], make_float4(q.px, q.py, q.pz, p.w));
                                else pts[myq] = make_float4(q.px, q.py, q.pz, p.w);
                            }
                            PipeSeed sd = {3.402823466e38f, 0, KeyFmt<KSH>::NONE};
                            if (it > 0) sd = seed_at<BIG>(BIG ? tp : s_tpl, take ? don_load(&nnq[myq]) : nnq[myq], q.px, q.py, q.pz);
                            if (it < 3) {   // coarse seeds: first point of every run
                                for (int j = 0; j < tpl_m; j += ICP_SUB) {
                                    const PipeSeed c = seed_at<BIG>(BIG ? tp : s_tpl, j, q.px, q.py, q.pz);
                                    if (c.d2 < sd.d2) sd = c;
                                }
                            }
                            q.pbest = seed_bound(sd.d2); q.pbi = sd.pos; kw = sd.kw;
                            CD_STAT_SEEDS(nk, it, tpl_m)
                        } else {            // final X <- T*X, then getFitnessScore() of Tfinal * original source
                            float ox, oy, oz;
                            xform(sl->so.T, p.x, p.y, p.z, ox, oy, oz);
                            pts[myq] = make_float4(ox, oy, oz, p.w);
                            const float4 p0 = pts0[myq];
                            xform(sl->so.Tfinal, p0.x, p0.y, p0.z, q.px, q.py, q.pz);
                            const PipeSeed sd = seed_at<BIG>(BIG ? tp : s_tpl, nnq[myq], q.px, q.py, q.pz);
                            q.pbest = seed_bound(sd.d2); q.pbi = sd.pos; kw = sd.kw;
                        }
                    }
                    CD_PHASE(1)
                    // search: the near queries (seed ball at most rmax wide) a lane each over the grid, the far ones a wave each
                    float rr = 0.f;
                    bool near = false;
                    if (lane < nk) { rr = __fmul_rn(__fsqrt_rn(q.pbest), 1.0f + 2.0e-6f); near = rr <= rmax; }
                    {
                        // from the seed BOUND (next float above d2(q, seed): what the radius of the walk is derived from) to the
                        // seed's own KEY for both searches: d2 exactly (the bound's bit pattern minus one) and the key word of the
                        // seed point; a query without a finite seed distance keeps (+inf, no index)
                        const unsigned bb = __float_as_uint(q.pbest);
                        const bool fin = bb < 0x7f800000u && lane < nk;
                        q.pbest = __uint_as_float(fin ? bb - 1u : bb);
                        q.poi = (int)(fin ? kw : KeyFmt<KSH>::NONE);
                    }
                    if (ballot64(near)) grid_search<KSH, !BIG, true>(BIG ? tp : s_tpl, s_cs, g, near, rr, q, gpad);
                    CD_STAT_NEAR(nk, near, lane < nk && !near && phase == PH_ITER, it, rr * g.inv)
                    CD_PHASE(2)
                    if constexpr (BIG) {
                        search_patches_big(tk, km, s_plo, s_phi, sp, q, ballot64(lane < nk && !near), &s_far[wave]);
                    } else {
                        search_patches(s_tpl, s_kd, bx, q, ballot64(lane < nk && !near), psplit, &s_far[wave], CD_IT_ACC);
                        CD_IT_END()
                    }
                    CD_STAT_REACH(lane < nk && !near && phase == PH_ITER, __fmul_rn(__fsqrt_rn(q.pbest), 1.0f + 2.0e-6f) <= rmax, it)
                    CD_PHASE(4)
                    pipe_fold_pass<BIG, BOUNDED>(sl, BIG ? tp : s_tpl, q, nk, phase, give, &nnq[myq], bnd.d2_max);
                    CD_PHASE(5)
                }
                CD_PHASE(5)
            }
            // arrive
            if (give) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the write-through stores of this wave have landed)
            __threadfence_block();
            int a = 0;
            if (lane == 0) a = atomicAdd(&sl->arrived, 1);
            a = __builtin_amdgcn_readfirstlane(a);
            if (a == ICPT_WAVES - 1) {   // last to arrive: finish the step for everybody
                __threadfence_block();
                if (lane == 0) {
                    if (phase == PH_ITER) {
                        if (pipe_end_iteration(sl, s_slot, st, don, prm)) { DON_DBG(24, don_t0); pipe_refill(sl, gbeg, gend, order, cl, st, queue, don, no_queue); }
                    } else {
                        if (phase == PH_FIT) {
                            sl->so.done = 1;
                            st[2 * (size_t)sl->k] = sl->so;
                            st[2 * (size_t)sl->k + 1] = sl->so;
                            accf[sl->k] = sl->acc[0];
                            if (don) __hip_atomic_fetch_add(don + DON_FINISHED, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        pipe_refill(sl, gbeg, gend, order, cl, st, queue, don, no_queue);
                    }
                    pipe_slot_clear<BOUNDED>(sl);
                }
                __threadfence_block();
                if (lane == 0) __hip_atomic_store(&sl->epoch, (want + 1) & 0xff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                CD_PHASE(3)
            }
            my_ep = (my_ep & ~(0xffull << (8 * sidx))) | ((unsigned long long)((want + 1) & 0xff) << (8 * sidx));
        }
    }
    // nothing left here.  With hand-overs on, wait for a running cluster of a workgroup that still has several (see pipe_give):
    // it goes into slot 0, whose step counter every wave left at the slot's current epoch.
    if (!don) break;
    __syncthreads();
    if (threadIdx.x == 0) {
        DON_DBG_WAIT_BEGIN
        const int k = pipe_wait_for_cluster(don, gend - gbeg, prm.don_fault ? (1 << 14) : (1 << 24));
        DON_DBG_WAIT_END(k)
        s_take = k;
        if (k >= 0) pipe_take_over<BOUNDED>(&s_slot[0], k, cl, st);
    }
    __syncthreads();
    if (s_take < 0) break;
    live = 1u;
    }
    CD_TIMERS_END
}

template <bool BOUNDED>
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_pipe(int ncl, const int* __restrict__ order,
                                                           const IcpCluster* __restrict__ cl, IcpState* st,
                                                           unsigned long long* __restrict__ accf,
                                                           const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                           const float4* __restrict__ thi,
                                                           const unsigned short* __restrict__ kdmap,
                                                           const IcpGrid* __restrict__ grids,
                                                           const unsigned short* __restrict__ tcell, float4* src,
                                                           const float4* __restrict__ src0, int* nn, int* queue,
                                                           const int* __restrict__ wgtab, IcpParams prm, IcpBound bnd) {
    icp_pipe_body<false, BOUNDED>(ncl, order, cl, st, accf, tpl, tlo, thi, kdmap, grids, tcell, src, src0, nn, queue, wgtab, prm, nullptr, nullptr, bnd);
}
template <bool BOUNDED>
__global__ void __launch_bounds__(ICPT_THREADS) k_icp_pipe_big(int ncl, const int* __restrict__ order,
                                                               const IcpCluster* __restrict__ cl, IcpState* st,
                                                               unsigned long long* __restrict__ accf,
                                                               const float4* __restrict__ tpl, const float4* __restrict__ tlo,
                                                               const float4* __restrict__ thi,
                                                               const unsigned short* __restrict__ kdmap,
                                                               const IcpGrid* __restrict__ grids,
                                                               const unsigned short* __restrict__ tcell, float4* src,
                                                               const float4* __restrict__ src0, int* nn, int* queue,
                                                               const int* __restrict__ wgtab, IcpParams prm,
                                                               const float4* __restrict__ tplk, const IcpSuper* __restrict__ supers, IcpBound bnd) {
    icp_pipe_body<true, BOUNDED>(ncl, order, cl, st, accf, tpl, tlo, thi, kdmap, grids, tcell, src, src0, nn, queue, wgtab, prm, tplk, supers, bnd);
}

void launch_icp_pipe(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_wg, const int* wgtab, IcpParams prm, const IcpBound& bnd) {
    if (ncl <= 0 || n_wg <= 0) return;
    hipLaunchKernelGGL(bnd.bounded ? k_icp_pipe<true> : k_icp_pipe<false>, dim3(n_wg), dim3(ICPT_THREADS), 0, s, ncl, P.order, P.cl, P.st, P.accf, T.tpl, T.tlok, T.thik,
                       T.kdmap, T.grids, T.tcell, S.src, S.src0, S.nn, S.queue, wgtab, prm, bnd);
}

void launch_icp_pipe_big(hipStream_t s, int ncl, const IcpProblems& P, const IcpTemplates& T, const IcpScratch& S, int n_wg, const int* wgtab, IcpParams prm, const IcpBound& bnd) {
    if (ncl <= 0 || n_wg <= 0) return;
    hipLaunchKernelGGL(bnd.bounded ? k_icp_pipe_big<true> : k_icp_pipe_big<false>, dim3(n_wg), dim3(ICPT_THREADS), 0, s, ncl, P.order, P.cl, P.st, P.accf, T.tpl, T.tlok, T.thik,
                       T.kdmap, T.grids, T.tcell, S.src, S.src0, S.nn, S.queue, wgtab, prm, T.tplk, T.supers, bnd);
}

}  // namespace cd
