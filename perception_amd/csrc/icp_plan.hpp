// icp_plan.hpp - the host arithmetic of the ICP stage (S6): which driver takes which cluster of a batch, and how each driver's
// launch is sized.  Plain inputs, plain outputs, no HIP runtime call and no context: icp_stage.hip feeds it from the context and
// issues the stream operations; icp_plan_check.cpp runs it on a CPU (tests/test_icp_plan_cpu.py).  The thresholds here are
// measurements; the comments that record them stay with the lines they explain.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "common.hpp"
#include "tunables.hpp"

namespace cd {

// What plan_icp reads of a context.  Counts that come from the per-device atomics (batches / calls in flight) are arguments of
// the functions that look at them: the caller loads each once.
struct IcpPlanInput {
    IcpCluster* cl = nullptr;            // the problems of the stage; plan_icp sets tile0 of each
    int ncl = 0;
    const int* tpl_faces = nullptr;      // per template slot: faces of its lattice (0: the generic searches take it)
    const bool* tpl_gridded = nullptr;   // per template slot: it has a cell start table
    const bool* tpl_big = nullptr;       // per template slot: it does not fit LDS but has what k_icp_pipe_big needs
    const Tunables* tun = nullptr;
    int n_cu = 256, work_cap = 0;        // CUs of the device; items the work list holds
    bool plane_on = false;               // rule C17 (cd_set_icp_plane_weight != 0)
    bool reject_on = false;              // rule C19 (cd_set_icp_median_rejection != 0)
    bool recip_on = false;               // rule C22 (cd_set_icp_reciprocal != 0)
    int icp_use_guess = CD_GUESS_NONE;   // cd_params::icp_use_guess
    const float* frame_guess = nullptr;  // the per-frame guesses in force (cd_set_frame_guesses', or - CD_GUESS_SURFACE - the call's own), 16 per frame
    size_t frame_guess_len = 0;          // floats
    const float* icp_guess = nullptr;    // cd_params::icp_guess, the single guess
    bool device_guesses = false;         // rule C18's fine stage: a kernel of the caller's writes one guess per problem on the device
                                         // (d_guess[16 k], Tfinal of d_st) after the states are up; the call's own guess is what a
                                         // problem it leaves alone starts from
};

struct PlanStatus { int code; const char* msg; };   // CD_OK, or what the caller fails the call with

// kind: 0 = no persistent kernel can take the template, 1 = k_icp_pipe (LDS-resident, gridded), 2 = k_icp_pipe_big (global memory)
inline int tpl_kind(const IcpPlanInput& in, const IcpCluster& cl) {
    if (cl.tpl_m <= 0 || !in.tpl_gridded[cl.slot]) return 0;
    if (cl.tpl_m <= ICP_TPL_LDS) return 1;
    return in.tpl_big[cl.slot] ? 2 : 0;
}

struct TplGroup { int beg, end, live; int kind; long long pts; };

struct IcpPlan {   // host-side decisions of one ICP stage (plan_icp)
    int ncl = 0, guess_mode = CD_GUESS_NONE, max_n = 0, qslice = 0;
    size_t guess_need = 0;                       // floats of the guess upload
    const float* frame_guess = nullptr;          // per-frame guesses (IcpPlanInput::frame_guess)
    std::vector<char> in_lat;                    // the cluster takes k_icp_lat
    int n_lat = 0, n_live = 0, lat_max_n = 0;
    int icp_search = -1;                         // cd_timing::icp_search: 0 generic searches, 1 closed form for every live cluster, 2 mixed (-1: not decided yet)
    std::vector<TplGroup> groups;
    int nwork = 0;                               // items of the sliced work list
    int wg_cap = 0;                              // workgroups of a persistent ICP launch at most (CUBOID_ICP_MAX_WG)
    bool grouped_pipe = false, lat_direct = false, pipe_ok = false, big_ok = false, whole_cluster = false;
    bool pre_zeroed = false;                     // (icp_setup) d_acc / d_accf / d_queue were zeroed by the fused call
    bool crowded = false;                        // (icp_params) four or more batches in flight on the device
    bool plane = false;                          // rule C17 (cd_set_icp_plane_weight): every live cluster takes k_icp_plane
    bool reject = false;                         // rule C19 (cd_set_icp_median_rejection): every live cluster gets sliced work items (icp_run_sliced)
    bool recip = false;                          // rule C22 (cd_set_icp_reciprocal): likewise, with k_icp_recip behind each iteration
    bool filtered() const { return reject || recip; }   // a kernel behind every k_icp_iter<true> replaces the slot's sums: the sliced loop only
    bool device_guesses = false;                 // (IcpPlanInput::device_guesses) the sources are moved per problem, whatever the guess mode
};

// Clusters in.cl[0..ncl) -> plan; fills the work list `work`, tile0 of every cluster and the initial states st[0 .. 2 * ncl).
inline PlanStatus plan_icp(const IcpPlanInput& in, IcpPlan* pl, IcpWork* work, IcpState* st_out) {
    const int ncl = in.ncl;
    const Tunables& tun = *in.tun;
    pl->ncl = ncl;
    // initial guess (pcl::Registration::align(output, guess)); the default - and the reference's live path - is none
    // (CD_GUESS_SURFACE is CD_GUESS_PER_FRAME with the guesses the call derived itself)
    const int guess_mode = pl->guess_mode = in.icp_use_guess == CD_GUESS_SURFACE ? CD_GUESS_PER_FRAME : in.icp_use_guess;
    pl->frame_guess = in.frame_guess;
    pl->device_guesses = in.device_guesses;
    if (guess_mode != CD_GUESS_NONE || in.device_guesses) {
        int max_frame = 0;
        for (int k = 0; k < ncl; ++k) { pl->max_n = std::max(pl->max_n, in.cl[k].n); max_frame = std::max(max_frame, in.cl[k].frame); }
        pl->guess_need = guess_mode == CD_GUESS_PER_FRAME ? 16 * ((size_t)max_frame + 1) : (guess_mode == CD_GUESS_CLUSTER ? 16 * (size_t)ncl : 16);
        if (guess_mode == CD_GUESS_PER_FRAME && in.frame_guess_len < pl->guess_need) return PlanStatus{CD_ERR_INVALID_ARG, "icp_use_guess = CD_GUESS_PER_FRAME but cd_set_frame_guesses holds fewer frames than the batch"};
        if (in.device_guesses) pl->guess_need = 16 * (size_t)ncl;   // (the device table replaces the upload)
    }
    // queries per workgroup: 512 when the batch fills the chip, smaller slices (more workgroups) otherwise
    long long qtot = 0;
    for (int k = 0; k < ncl; ++k) qtot += in.cl[k].n;
    pl->qslice = std::max(64, std::min(ICP_QSLICE, (int)((qtot / 512 + 15) / 16 * 16)));
    // Template groups: runs of clusters that share a template (one run per template when every cluster is matched against
    // every template).  With several templates in the batch, the groups whose template is LDS-resident and gridded go through
    // ONE k_icp_pipe launch (each group gets a share of the workgroups and its own queue) when there are enough of them to
    // fill a fifth of the chip; the other clusters take the sliced driver.
    // Clusters whose template is a lattice (every make_cuboid.py template; IcpLattice, common.hpp) go to k_icp_lat - closed-form
    // nearest neighbour, one workgroup per cluster - and take no part in the grouping.  CUBOID_ICP_LATTICE=0 and the
    // forced driver modes (CUBOID_ICP_MODE) keep them on the generic searches (A/B, and the GPU suite runs under each mode).
    // Rule C17 on: every live cluster goes to k_icp_plane whatever those switches say - no other driver implements the step.
    // Rule C19 on: every live cluster takes the sliced loop with k_icp_reject behind each iteration, likewise whatever they say.
    // Rule C22 on: the same with k_icp_recip.
    pl->plane = in.plane_on;
    pl->reject = in.reject_on;
    pl->recip = in.recip_on;
    if (pl->plane && pl->reject) return PlanStatus{CD_ERR_INVALID_ARG, "plane-weighted ICP and median-distance rejection are both on"};
    if (pl->recip && (pl->plane || pl->reject)) return PlanStatus{CD_ERR_INVALID_ARG, "reciprocal correspondences and plane-weighted ICP or median-distance rejection are both on"};
    const bool use_lat = !pl->plane && !pl->filtered() && tun.icp_lattice != 0 && tun.icp_mode == 0;
    pl->in_lat.assign((size_t)ncl, 0);
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = in.cl[k];
        const bool live = cl.n >= 3 && cl.tpl_m > 0;
        pl->n_live += live ? 1 : 0;
        if (pl->plane && live && in.tpl_faces[cl.slot] <= 0) return PlanStatus{CD_ERR_INVALID_ARG, "plane-weighted ICP is on and a template of the call is not a lattice"};
        if (use_lat && live && in.tpl_faces[cl.slot] > 0) { pl->in_lat[(size_t)k] = 1; ++pl->n_lat; pl->lat_max_n = std::max(pl->lat_max_n, cl.n); }
    }
    pl->icp_search = pl->plane ? 1 : (pl->n_lat == 0 ? 0 : (pl->n_lat == pl->n_live ? 1 : 2));
    std::vector<TplGroup>& groups = pl->groups;
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = in.cl[k];
        if (groups.empty() || in.cl[groups.back().beg].tpl_off != cl.tpl_off || in.cl[groups.back().beg].tpl_m != cl.tpl_m)
            groups.push_back(TplGroup{k, k, 0, use_lat && in.tpl_faces[cl.slot] > 0 ? 0 : tpl_kind(in, cl), 0});
        TplGroup& g = groups.back();
        g.end = k + 1;
        if (cl.n >= 3) { g.live += 1; g.pts += cl.n; }
    }
    int n_grouped = 0;
    for (const TplGroup& g : groups) if (g.kind) n_grouped += g.live;
    pl->grouped_pipe = !pl->plane && !pl->filtered() && groups.size() > 1 && groups.size() <= 16 && n_grouped > 0 &&
                       (tun.icp_mode == 3 || (tun.icp_mode == 0 && n_grouped * 5 >= in.n_cu));
    if (std::getenv("CUBOID_DEBUG")) {
        std::fprintf(stderr, "cuboid_hip: stage_icp %d clusters, %zu template groups, %d in pipe groups, grouped_pipe %d:", ncl, groups.size(), n_grouped, (int)pl->grouped_pipe);
        for (const TplGroup& g : groups) std::fprintf(stderr, " [%d,%d) m=%d kind=%d live=%d", g.beg, g.end, in.cl[g.beg].tpl_m, g.kind, g.live);
        std::fprintf(stderr, "\n");
    }
    std::vector<char> in_pipe((size_t)ncl, 0);
    if (pl->grouped_pipe)
        for (const TplGroup& g : groups) if (g.kind) for (int k = g.beg; k < g.end; ++k) in_pipe[(size_t)k] = 1;
    int nwork = 0;
    for (int k = 0; k < ncl; ++k) {
        IcpCluster& cl = in.cl[k];
        cl.tile0 = nwork;
        const int tiles = cl.n >= 3 && cl.tpl_m > 0 && !in_pipe[(size_t)k] && !pl->in_lat[(size_t)k] && !pl->plane ? (cl.n + pl->qslice - 1) / pl->qslice : 0;
        if (nwork + tiles > in.work_cap) return PlanStatus{CD_ERR_CAPACITY, "ICP work list overflow"};
        for (int t = 0; t < tiles; ++t) work[nwork++] = IcpWork{k, t};
        for (int s = 0; s < 2; ++s) {
            IcpState& st = st_out[2 * k + s];
            std::memset(&st, 0, sizeof(st));
            for (int i = 0; i < 4; ++i) st.Tfinal[5 * i] = 1.f;
            if (guess_mode != CD_GUESS_NONE && guess_mode != CD_GUESS_CLUSTER)   // final_transformation_ = guess (CD_GUESS_CLUSTER: k_shape_frames writes it on the device)
                std::memcpy(st.Tfinal, guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess + 16 * (size_t)cl.frame : in.icp_guess, 64);
            st.prev_mse = std::numeric_limits<double>::max();
            if (cl.tpl_m <= 0) { st.done = 1; st.status = CD_ERR_NO_TEMPLATE; }
            else if (cl.n < 3) { st.done = 1; st.status = CD_ERR_FEW_CORRESPONDENCES; }
        }
    }
    pl->nwork = nwork;
    pl->wg_cap = tun.icp_max_wg > 0 ? std::min(tun.icp_max_wg, in.n_cu) : in.n_cu;
    // A stage whose clusters ALL take k_icp_lat (the default template, no initial guess): the kernel reads the cluster list, the
    // order and the initial states from the pinned host arrays and writes the final states and fitness sums there - a few
    // hundred bytes per cluster once at each end of its ICP - instead of three copy launches around it.
    pl->lat_direct = tun.icp_direct && pl->n_lat > 0 && pl->n_lat == pl->n_live && guess_mode == CD_GUESS_NONE && !in.device_guesses && tun.mirror_reads && tun.mirror_writes && tun.copy_kernels;
    // Batch mode: with at least ~n_cu/5 clusters every CU can own whole clusters, so each cluster runs its
    // complete ICP (all iterations + fitness) inside one persistent workgroup, one launch for the batch.
    // The pipelined variant (two to four clusters in flight per workgroup, no barrier in the iteration loop) needs one
    // LDS-resident gridded template shared by every cluster of the launch; otherwise k_icp_cluster runs.
    bool one_tpl = true;
    for (int k = 1; k < ncl && one_tpl; ++k) one_tpl = in.cl[k].tpl_off == in.cl[0].tpl_off && in.cl[k].tpl_m == in.cl[0].tpl_m;
    pl->pipe_ok = tun.icp_mode != 2 && one_tpl && tpl_kind(in, in.cl[0]) == 1;
    // ... or, for a template that does not fit LDS, its twin that reads the template from global memory (k_icp_pipe_big)
    pl->big_ok = tun.icp_mode != 2 && one_tpl && tpl_kind(in, in.cl[0]) == 2;
    // (auto mode: only the pipelined kernel beats the sliced driver; with mixed or non-resident templates k_icp_cluster's
    // barrier per iteration costs more than it saves, so those batches stay sliced unless the mode is forced)
    // (measured crossover on the bench frames: 33 clusters 3.3 ms sliced / 3.7 ms pipelined, 65 clusters 4.4 / 3.9, 130 clusters
    // 6.4 / 4.0: the pipelined kernel wins from about a fifth of the CUs' worth of clusters)
    pl->whole_cluster = !pl->grouped_pipe && !pl->filtered() && (tun.icp_mode >= 2 || (tun.icp_mode == 0 && ncl * 5 >= in.n_cu && (pl->pipe_ok || pl->big_ok)));
    return PlanStatus{CD_OK, nullptr};
}

// which guess k_icp_apply_guess moves problem k by: the only one, its frame's, its own
inline int guess_indexing(int guess_mode) { return guess_mode == CD_GUESS_PER_FRAME ? 1 : (guess_mode == CD_GUESS_CLUSTER ? 2 : 0); }
// ... of a planned stage: its own with guesses written per problem on the device (IcpPlanInput::device_guesses); -1: the sources stay
inline int guess_indexing(const IcpPlan& pl) { return pl.device_guesses ? 2 : (pl.guess_mode == CD_GUESS_NONE ? -1 : guess_indexing(pl.guess_mode)); }

// the cluster order of every queue-fed launch: order[0..no) sorted largest first, equal sizes in the order they came in
inline void largest_first(int* order, int no, const IcpCluster* cl) {
    std::stable_sort(order, order + no, [&](int a, int b) { return cl[a].n > cl[b].n; });
}

// Shape of the k_icp_lat launch (k_icp_lat.hip): clusters per workgroup x waves per cluster.  A call that has the GPU to itself
// wants the launch short: one cluster per workgroup, four waves each when there are clusters enough to fill the chip twice that
// way, eight or sixteen for fewer or very large clusters (one frame; config 5's thousands of points).  With other batches in
// flight the chip is full anyway: four clusters per workgroup, two waves each, pay the single-lane solve of a round once
// for the four (measured on config 3, seven in flight, profiles/r05_lat_shapes.txt: 1x4 145-146 k, 4x2 149-151 k, 8x2 146 k,
// 4x4 139 k, 4x1 131 k frames/s; alone 1x4 1.34 ms, 1x8 1.30, 4x2 2.2, 4x1 2.8).  CUBOID_LAT_SHAPE=cpw,wpc[,clusters per slot].
struct LatShape { int cpw, wpc, per_slot, n_wg; };
inline LatShape lat_launch_shape(int n_lat, int lat_max_n, int batches_in_flight, const int lat_shape[3]) {
    const bool busy = batches_in_flight >= 3;
    int cpw = 1, wpc = n_lat >= 768 ? 4 : (n_lat >= 96 ? 8 : 16), per_slot = 1;   // (end of round 5, 522 clusters alone: 1x4 1.17 ms, 1x8 1.10, 1x16 1.53, 2x4 1.27)
    if (lat_max_n > 16384) wpc = 16;
    else if (lat_max_n > 4096) wpc = std::max(wpc, 8);
    if (busy && n_lat >= 256 && lat_max_n <= 8192) { cpw = 4; wpc = 2; }
    if (lat_shape[0] > 0) { cpw = lat_shape[0]; wpc = std::max(1, lat_shape[1]); per_slot = std::max(1, lat_shape[2]); }
    const int n_wg = std::max(1, (n_lat + cpw * per_slot - 1) / (cpw * per_slot));
    return LatShape{cpw, wpc, per_slot, n_wg};
}

// workgroups of the k_icp_plane launch over `no` clusters: two per CU at the most - 256 registers a wave leave two waves per
// SIMD (k_icp_plane.hip)
inline int plane_launch_grid(int no, int wg_cap) { return std::max(1, std::min(no, 2 * wg_cap)); }

// The launch of the template groups of a several-template batch (plan.grouped_pipe).  Items of `order`: the pipe groups one
// after the other (those of k_icp_pipe first, then those of k_icp_pipe_big), each largest cluster first.  The two kernels are
// launched side by side (second stream): their workgroups share the chip, every group gets workgroups in proportion to its
// points (a query against a template in global memory counted BIG_WEIGHT times), at least one, no more than it has clusters.
// tab: {first item, end item, queue} per workgroup, 1024 rows at the most; wg_of / tab_of[kind]: the workgroups of kernel
// `kind` (1 k_icp_pipe, 2 k_icp_pipe_big) and where its rows start in tab; share[q]: the workgroups of queue q.
struct GroupedLaunch { long long big_weight; int no, ntab, n_wg, nq, wg_of[3], tab_of[3], share[16]; };
inline GroupedLaunch grouped_launch_table(const std::vector<TplGroup>& groups, const IcpCluster* cl, int wg_cap, const Tunables& tun, int* order, int* tab) {
    GroupedLaunch L = {0, 0, 0, 0, 0, {0, 0, 0}, {0, 0, 0}, {0}};
    // (while every problem can have a workgroup of its own the launch lasts as long as its longest cluster, and those are the
    // global-memory ones: 4; with more problems than workgroups it is their throughput that counts, 1.6 x the LDS kernel's
    // cost per workgroup plus the longer tail: 2 - config 5 at 8 frames per batch 4 > 2 by 5 %, at 64 frames 2 > 4 by 6 %)
    int live_all = 0;
    for (const TplGroup& g : groups) if (g.kind) live_all += g.live;
    const long long BIG_WEIGHT = L.big_weight = tun.icp_big_weight > 0 ? tun.icp_big_weight : (live_all <= wg_cap ? 4 : 2);
    const int cpw = std::max(1, tun.icp_cpw);   // (0 = default: a group may have as many workgroups as clusters)
    int ntab = 0;
    long long pts_all = 0;
    int npg = 0;
    for (const TplGroup& g : groups) if (g.kind && g.live > 0) { pts_all += g.pts * (g.kind == 2 ? BIG_WEIGHT : 1); ++npg; }
    int no = 0, gq = 0, n_wg = 0;
    for (int kind = 1; kind <= 2; ++kind) {
        L.tab_of[kind] = ntab;
        for (const TplGroup& g : groups) {
            if (g.kind != kind || g.live == 0) continue;
            const int b = no;
            for (int k = g.beg; k < g.end; ++k) if (cl[k].n >= 3) order[no++] = k;
            largest_first(order + b, no - b, cl);
            int share = (int)((long long)wg_cap * g.pts * (kind == 2 ? BIG_WEIGHT : 1) / std::max(pts_all, 1ll));
            share = std::max(1, std::min(share, std::min((g.live + cpw - 1) / cpw, wg_cap - n_wg - (npg - 1 - gq))));
            for (int w = 0; w < share && ntab + 3 <= 3 * 1024; ++w) { tab[ntab++] = b; tab[ntab++] = no; tab[ntab++] = gq; }
            n_wg += share;
            L.wg_of[kind] += share;
            if (gq < 16) L.share[gq] = share;
            ++gq;
        }
    }
    L.no = no; L.ntab = ntab; L.n_wg = n_wg; L.nq = gq;
    return L;
}

// Whole-cluster launches: how many clusters a workgroup keeps in flight and how many workgroups there are.  A call that has
// the device to itself wants every CU at work: one workgroup per CU (or per cluster), two slots, the second filled as long
// as clusters are left.  With other calls in flight (BatchPipeline) the chip is full anyway and what counts is the CU-time
// a batch costs: FOUR clusters per workgroup keep its sixteen waves supplied while one of them solves a step (no wave waits
// at a hand-over, no workgroup ends with one cluster alone), on a quarter as many workgroups - the other batches have the
// other CUs (config 3, 522 clusters: 2 x 256 -> 4 x 128 is 48.4 -> 53.3 k frames/s; grids that are not a multiple of 32 -
// 4 per XCD and shader engine - lose 2-4 %).
// (crossover measured on config 3: with two calls in flight the two shapes tie, with three 2 x 256 wins 49.4 : 46.5 k, with
// four 4 x 128 wins 52.9 : 49.7 k - and the last launches of a burst, which soon have the GPU to themselves, spread out)
inline bool icp_crowded(int batches_in_flight) { return batches_in_flight >= 4; }
// (grouped: template groups keep two clusters in flight per workgroup whatever the regime: every group has its share of the
// workgroups and its own queue already, and four slots measure 3-7 % slower on config 5)
inline int pipe_slots(int icp_slots, bool crowded, bool grouped) {
    if (icp_slots > 0) return std::min(icp_slots, CD_PIPE_SLOTS);
    return crowded && !grouped ? CD_PIPE_SLOTS : std::min(2, CD_PIPE_SLOTS);
}

// workgroups of a whole-cluster launch over n_items clusters
inline int whole_launch_grid(int n_items, int cap, int icp_cpw, bool crowded, int slots) {
    if (icp_cpw > 0) return std::min((n_items + icp_cpw - 1) / icp_cpw, cap);
    if (!crowded || n_items <= cap) return std::min(n_items, cap);
    return std::min(cap, std::max(32, (n_items / slots + 16) / 32 * 32));
}

// A launch that has the GPU to itself lets workgroups that run out of clusters wait and take over running ones
// (k_icp_pipe.hip, "hand-over of running clusters"): the launch is as long as its slowest workgroup, and the bench batch's
// slowest runs 25 % over the average.  With other calls in flight a waiting workgroup would sit on a CU their
// kernels could use, and what counts there is the CU-time a batch costs, which hand-overs do not lower.
inline bool whole_donate(int icp_donate, int batches_in_flight, int ncl, int grid) {
    const bool alone = batches_in_flight <= 1;
    return icp_donate < 0 ? (alone && ncl > grid) : icp_donate != 0;
}

// Few clusters: ONE persistent launch of G workgroups runs every iteration and the fitness pass; n_open: the clusters that have
// work items (k_icp_persist's exit test).
// (with other contexts at work - BatchPipeline - their persistent kernels hold the CUs this launch's grid barrier needs:
// it would wait, give up and hand over; go straight to the multi-launch loop then)
// measured against the multi-launch loop: 1 frame 1.50 / 1.78 ms, 4 frames 1.94 / 2.36, 8 frames 3.04 / 2.66 - with many
// clusters the launch lasts as long as the slowest one while finished workgroups wait at the barriers, and a workgroup
// with several items solves for each of them in turn
struct PersistLaunch { bool launch; int G, n_open; };
inline PersistLaunch persist_launch(const IcpCluster* cl, int ncl, int nwork, int wg_cap, int icp_persist, int calls_in_flight) {
    const bool siblings = calls_in_flight > 1;
    if (nwork == 0 || !icp_persist || (siblings && icp_persist != 2)) return PersistLaunch{false, 0, 0};
    const int G = std::min(nwork, wg_cap);
    if (ncl > 8 || nwork > G) return PersistLaunch{false, G, 0};
    int n_open = 0;
    for (int k = 0; k < ncl; ++k) if (cl[k].tile0 < (k + 1 < ncl ? cl[k + 1].tile0 : nwork)) ++n_open;
    return PersistLaunch{true, G, n_open};
}

// iteration launches the sliced driver issues between two completion polls: 8 before the first poll, 16 after it
inline int sliced_poll_group(int polls_done) { return polls_done == 0 ? 8 : 16; }

// The sliced driver's active work list after a completion poll: the items of `work` whose cluster is done in neither parity slot
// (a cluster whose state shows done in either slot has already had its final transform applied), in their order.  Returns their
// count; *all_done: every cluster is done in both slots.
inline int repack_active(const IcpWork* work, int nwork, const IcpState* st, int ncl, IcpWork* active, bool* all_done) {
    bool all = true;
    int na = 0;
    for (int w = 0; w < nwork; ++w) {
        const int k = work[w].cluster;
        if (!(st[2 * k].done || st[2 * k + 1].done)) active[na++] = work[w];
    }
    for (int k = 0; k < ncl && all; ++k) all = st[2 * k].done && st[2 * k + 1].done;
    *all_done = all;
    return na;
}

}  // namespace cd
