// icp_stage.hip - S6, the ICP stage: stage_icp plans the stage on the host (plan_icp, icp_plan.hpp), issues what every driver
// needs (icp_setup), then hands the clusters to the drivers in turn: k_icp_lat for lattice templates, the grouped k_icp_pipe
// launches for several templates (k_icp_pipe.hip), the whole-cluster launch (k_icp_pipe.hip, k_icp_cluster.hip), the persistent
// launch for a few clusters and the sliced multi-launch loop for whatever is left (both k_icp.hip).
// Rule C17 on: k_icp_plane takes every live cluster and finishes the stage; none of the others runs.
// Rule C19 on: the sliced loop, with k_icp_reject behind every iteration, takes every live cluster; none of the others runs.
// Rule C22 on: the same with k_icp_recip.
// A driver sets *done when it has run the stage to its end (records read back, stream synchronised); otherwise the drivers after
// it take the clusters it left and find the ones it ran finished in d_st / h_st (the stream orders them).
// Which driver, and how large its launch: icp_plan.hpp decides, from plain numbers.  Here are the stream operations.
#include "context.hpp"
#include "host_math.hpp"
#include "icp_plan.hpp"

namespace {

// plan_icp over the context: the clusters h_cl[0..ncl) -> plan; fills h_work, tile0 of every cluster and the initial states h_st
int plan_stage(cd_context* c, int ncl, const cd_params* p, bool device_guesses, IcpPlan* pl) {
    IcpPlanInput in;
    in.cl = c->h_cl; in.ncl = ncl;
    in.tpl_faces = c->tpl_faces; in.tpl_gridded = c->tpl_gridded; in.tpl_big = c->tpl_big;
    in.tun = &c->tun; in.n_cu = c->n_cu; in.work_cap = c->work_cap;
    in.plane_on = c->plane_weight != 0.0;
    in.reject_on = c->reject_factor != 0.0;
    in.recip_on = c->recip_on != 0;
    in.icp_use_guess = p->icp_use_guess;
    const std::vector<float>& fg = p->icp_use_guess == CD_GUESS_SURFACE ? c->surface_guess : c->frame_guess;
    in.frame_guess = fg.data(); in.frame_guess_len = fg.size();
    in.icp_guess = p->icp_guess;
    in.device_guesses = device_guesses;   // rule C18's fine stage (stage_icp_levels)
    const PlanStatus ps = plan_icp(in, pl, c->h_work, c->h_st);
    if (pl->icp_search >= 0) c->timing.icp_search = pl->icp_search;
    return ps.code == CD_OK ? CD_OK : fail(c, ps.code, ps.msg);
}

// The argument blocks of the ICP launchers (kernels.hpp), built once per stage after icp_setup has sized the buffers.  pinned:
// the problem set as k_icp_lat's direct mode reads and writes it.
struct IcpArgs { IcpProblems dev, pinned; IcpTemplates tpl; IcpScratch scr; };
IcpArgs icp_args(const cd_context* c) {
    IcpArgs a;
    a.dev = IcpProblems{c->d_order, c->d_cl, c->d_st, c->d_accf};
    a.pinned = IcpProblems{c->h_order, c->h_cl, c->h_st, c->h_accf};
    a.tpl = IcpTemplates{c->d_tpl, c->d_tplk, c->d_tlo, c->d_thi, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_super, c->d_tcell, c->d_lat};
    a.scr = IcpScratch{c->d_src, c->d_src0, c->d_nn, c->d_d2, c->d_acc, c->d_queue};
    return a;
}

// CD_GUESS_CLUSTER: k_shape_frames over the stage's ncl problems (d_cl, d_src0) -> d_shape, d_guess and Tfinal of d_st.  The
// template table goes up first when a template has changed since the last time (a copy launch from its pinned mirror: no
// synchronisation).  The buffers have been sized by icp_setup.
int launch_cluster_guesses(cd_context* c, int ncl) {
    if (c->tframe_dirty) {
        for (int s = 0; s < CD_MAX_TEMPLATES; ++s) c->h_tframe[s] = template_frame(c, s);
        HIPCHK(c, xfer(c, c->d_tframe, c->h_tframe, sizeof(ShapeFrame) * CD_MAX_TEMPLATES, hipMemcpyHostToDevice));
        c->tframe_dirty = false;
    }
    LAUNCH(c, launch_shape_frames(c->stream, ncl, c->d_cl, c->d_src0, c->d_shape, c->d_tframe, c->d_guess, c->d_st));
    return CD_OK;
}

// Rule C18, the fine stage (plan.device_guesses): per problem T_c or the call's own guess into d_guess and Tfinal of d_st, from the
// tables stage_icp_levels has put on the stream; the stats follow to their mirror (on the host by the stage's final synchronisation)
int launch_coarse_handover(cd_context* c, int ncl) {
    static_assert(sizeof(CoarseStats) == sizeof(cd_icp_coarse_stats), "CoarseStats mirrors cd_icp_coarse_stats");
    LAUNCH(c, launch_icp_coarse_handover(c->stream, ncl, c->d_chand, c->d_cst, c->d_caccf, c->d_st, c->d_guess, c->d_cstat));
    HIPCHK(c, xfer(c, c->h_cstat, c->d_cstat, sizeof(CoarseStats) * (size_t)ncl, hipMemcpyDeviceToHost));
    return CD_OK;
}

// the stream operations every driver needs before the stage's start event: guess, cluster list, work list, initial states,
// zeroed sums, guess applied to the sources
int icp_setup(cd_context* c, const cd_params* p, IcpPlan* pl) {
    const int ncl = pl->ncl, moved_by = guess_indexing(*pl);
    if (moved_by >= 0) {
        GROW(c, d_guess, pl->guess_need);
        if (pl->guess_mode == CD_GUESS_CLUSTER) {   // (the guesses are written on the device; the records' buffers before anything is on the stream)
            GROW(c, d_shape, (size_t)ncl); GROW(c, h_shape, (size_t)ncl);
            GROW(c, d_tframe, (size_t)CD_MAX_TEMPLATES); GROW(c, h_tframe, (size_t)CD_MAX_TEMPLATES);
        } else if (!pl->device_guesses)
            HIPCHK(c, copy_sync(c, c->d_guess, pl->guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess : p->icp_guess, sizeof(float) * pl->guess_need, hipMemcpyHostToDevice));
    }
    if (!pl->lat_direct) {
        XferBatch xb(c);   // (one launch)
        xb.add(c->d_cl, c->h_cl, sizeof(IcpCluster) * ncl, hipMemcpyHostToDevice);
        if (pl->nwork > 0) xb.add(c->d_work, c->h_work, sizeof(IcpWork) * pl->nwork, hipMemcpyHostToDevice);
        xb.add(c->d_st, c->h_st, sizeof(IcpState) * 2 * ncl, hipMemcpyHostToDevice);
        HIPCHK(c, xb.flush());
    }
    // (zeroed up front by the fused call for its FIRST ICP stage only: a batch that runs one stage per template fills them again)
    pl->pre_zeroed = c->batch_zeroed;
    c->batch_zeroed = false;
    if (!pl->pre_zeroed) {
        HIPCHK(c, hipMemsetAsync(c->d_acc, 0, sizeof(unsigned long long) * 48 * (size_t)ncl, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_accf, 0, sizeof(unsigned long long) * ((size_t)ncl + 1), c->stream));   // (+ the wave-time word of k_icp_lat)
    }
    if (c->icp_bounded || pl->filtered()) {   // rule C8: the sliced / persistent drivers' correspondence counts, [cluster][it % 3] (rules C19, C22: always)
        GROW(c, d_ncorr, 3 * (size_t)ncl);
        HIPCHK(c, hipMemsetAsync(c->d_ncorr, 0, sizeof(uint32_t) * 3 * (size_t)ncl, c->stream));
    }
    if (pl->guess_mode == CD_GUESS_CLUSTER) {   // rule C13: record, guess and Tfinal of every problem, after the d_cl / d_st upload above
        if (int e = launch_cluster_guesses(c, ncl)) return e;
        HIPCHK(c, xfer(c, c->h_shape, c->d_shape, sizeof(ShapeFrame) * (size_t)ncl, hipMemcpyDeviceToHost));   // (on the host by the stage's final synchronisation)
    }
    if (pl->device_guesses)   // rule C18: after the d_st upload and rule C13's guesses, which a problem that falls back keeps
        if (int e = launch_coarse_handover(c, ncl)) return e;
    if (moved_by >= 0)   // input_transformed = guess * source (d_src is a copy of d_src0 at this point)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl->max_n, c->d_cl, c->d_guess, moved_by, c->d_src0, c->d_src));
    return CD_OK;
}

// (crowded, and the slots of a whole-cluster launch with it: icp_plan.hpp)
IcpParams icp_params(const cd_context* c, const cd_params* p, bool* crowded) {
    IcpParams ip;
    ip.max_iter = p->icp_max_iterations;
    ip.grid_rc = 1.0f;
    if (const char* e = std::getenv("CUBOID_ICP_GRID_RC")) ip.grid_rc = (float)std::atof(e);
    ip.trans_eps = p->icp_transformation_epsilon;
    ip.rel_mse = p->icp_euclidean_fitness_epsilon;
    ip.rot_thr = 1.0 - p->icp_transformation_epsilon;
    ip.abs_mse = 1e-12;
    *crowded = icp_crowded(device_shared(c).batches_in_flight.load());
    ip.pipe_slots = pipe_slots(c->tun.icp_slots, *crowded, /*grouped=*/false);
    ip.donate = 0;   // (set by icp_run_whole for a launch that has the GPU to itself)
    ip.don = c->d_don;
    ip.don_idle = c->tun.don_idle;
    ip.don_fault = c->tun.don_fault;
    return ip;
}

// rule C8: every driver runs its BOUNDED instantiation when the context's distance bounds anything (after icp_setup, which
// sizes d_ncorr)
IcpBound icp_bound(const cd_context* c) {
    IcpBound b;
    b.d2_max = c->icp_d2_max;
    b.bounded = c->icp_bounded;
    b.ncorr = c->d_ncorr;
    return b;
}

// The read-back that ends a stage, for the drivers whose last stream operations are the same: the fitness sums, then the states,
// then the host waits.  (The others differ by what the order of their operations forbids to move: icp_run_whole copies the
// hand-over words before it waits, the lattice and plane drivers send their records as one XferBatch.)  The caller has recorded ev[6].
int icp_read_back(cd_context* c, int ncl) {
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CD_OK;
}

// after the host synchronise of the driver that ended the stage: the launch time (ev[5] -> ev[6]) and the point pairs tested
void icp_finish(cd_context* c, int ncl, long long* pair_tests) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[6]);
    c->timing.icp_kernel_ms = ms;
    if (pair_tests) {
        long long tot = 0;
        for (int k = 0; k < ncl; ++k)
            if (c->h_st[2 * k].status == CD_OK) tot += (long long)c->h_cl[k].n * c->h_cl[k].tpl_m * (c->h_st[2 * k].iters + 1);
        *pair_tests = tot;
    }
}

// k_icp_lat over the clusters whose template is a lattice; on a mixed batch the states come back for the drivers below.
int icp_run_lat(cd_context* c, const IcpPlan& pl, const IcpArgs& a, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, n_lat = pl.n_lat;
    // the clusters of the launch, largest first
    int no = 0;
    for (int k = 0; k < ncl; ++k) if (pl.in_lat[(size_t)k]) c->h_order[no++] = k;
    largest_first(c->h_order, no, c->h_cl);
    if (!pl.lat_direct) HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    const LatShape ls = lat_launch_shape(n_lat, pl.lat_max_n, device_shared(c).batches_in_flight.load(), c->tun.lat_shape);
    GateHold lat_hold;   // (CUBOID_ICP_CONCURRENT: at most that many contexts between this launch and its completion)
    if (c->tun.icp_concurrent > 0) lat_hold.enter(&device_shared(c).icp_gate, c->tun.icp_concurrent);
    if (!pl.pre_zeroed) HIPCHK(c, hipMemsetAsync(c->d_queue, 0, 2 * sizeof(int), c->stream));   // head of the cluster queue, count of finished workgroups
    if (pl.lat_direct) std::memset(c->h_accf, 0, sizeof(unsigned long long) * ((size_t)ncl + 1));   // (what the zeroed device array used to bring back for clusters the kernel skips)
    LAUNCH(c, launch_icp_lat(c->stream, n_lat, ls.cpw, ls.wpc, ls.n_wg, pl.lat_direct ? a.pinned : a.dev, a.tpl, a.scr, c->d_accf + ncl, pl.lat_direct ? c->h_accf + ncl : nullptr, ip, icp_bound(c)));
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (ls.cpw << 16) | std::min(ls.n_wg, 0xffff);
    if (n_lat < pl.n_live) {   // mixed batch
        HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    if (!pl.lat_direct) {
        XferBatch xb(c);   // (one launch)
        xb.add(c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost);
        xb.add(c->h_accf, c->d_accf, sizeof(unsigned long long) * ((size_t)ncl + 1), hipMemcpyDeviceToHost);
        HIPCHK(c, xb.flush());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->timing.icp_wave_ms = (float)((double)c->h_accf[ncl] / 1.0e5);   // 100 MHz ticks x waves -> wave-milliseconds
    *done = true;
    return CD_OK;
}

// Rule C17 (cd_set_icp_plane_weight): k_icp_plane over every live cluster of the stage, whatever its template slot - one
// launch, queue-fed, largest first; the ordinary device buffers (no pinned arrays read by the kernel).  Always finishes the stage.
int icp_run_plane(cd_context* c, const IcpPlan& pl, const IcpArgs& a, const IcpParams& ip, bool* done) {
    static_assert(sizeof(PlaneStats) == sizeof(cd_icp_plane_stats), "PlaneStats mirrors cd_icp_plane_stats");
    const int ncl = pl.ncl;
    int no = 0;
    for (int k = 0; k < ncl; ++k) if (c->h_cl[k].n >= 3 && c->h_cl[k].tpl_m > 0) c->h_order[no++] = k;
    largest_first(c->h_order, no, c->h_cl);
    GROW(c, d_pstat, (size_t)ncl); GROW(c, h_pstat, (size_t)ncl);
    if (no > 0) HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_pstat, 0, sizeof(PlaneStats) * (size_t)ncl, c->stream));   // (pre-marked problems keep zeros)
    if (!pl.pre_zeroed) HIPCHK(c, hipMemsetAsync(c->d_queue, 0, 2 * sizeof(int), c->stream));   // head of the cluster queue
    PlaneParams pp;
    pp.lambda = (float)c->plane_weight;
    pp.latched0 = std::isinf(c->plane_switch) ? 1 : 0;
    pp.switch2 = c->plane_switch * c->plane_switch;
    const int n_wg = plane_launch_grid(no, pl.wg_cap);
    LAUNCH(c, launch_icp_plane(c->stream, no, n_wg, a.dev, c->d_pstat, a.tpl, a.scr, ip, icp_bound(c), pp));
    c->timing.icp_kernel_launches = no > 0 ? 1 : 0;
    c->timing.icp_regime = (1 << 16) | std::min(n_wg, 0xffff);
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    {
        XferBatch xb(c);   // (one launch)
        xb.add(c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost);
        xb.add(c->h_accf, c->d_accf, sizeof(unsigned long long) * (size_t)ncl, hipMemcpyDeviceToHost);
        xb.add(c->h_pstat, c->d_pstat, sizeof(PlaneStats) * (size_t)ncl, hipMemcpyDeviceToHost);
        HIPCHK(c, xb.flush());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;
    return CD_OK;
}

// The template groups of a several-template batch (plan.grouped_pipe): k_icp_pipe and k_icp_pipe_big side by side (their shares
// of the workgroups: grouped_launch_table); the stage is finished when no cluster is left for the sliced driver.
int icp_run_grouped(cd_context* c, const IcpPlan& pl, const IcpArgs& a, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl;
    IcpParams ipg = ip;
    ipg.pipe_slots = pipe_slots(c->tun.icp_slots, pl.crowded, /*grouped=*/true);
    int* tab = c->h_wgtab;   // pinned: the copy below is asynchronous
    const GroupedLaunch gl = grouped_launch_table(pl.groups, c->h_cl, pl.wg_cap, c->tun, c->h_order, tab);
    const int* wg_of = gl.wg_of;
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)gl.no, hipMemcpyHostToDevice));
    HIPCHK(c, xfer(c, c->d_wgtab, tab, sizeof(int) * (size_t)gl.ntab, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int) * 16, c->stream));   // one queue head per group
    // the LDS-template launch goes to the context's stream (stream3 with icp_lowprio), the global-template launch beside it
    hipStream_t s1 = c->tun.icp_lowprio ? c->stream3 : c->stream;
    hipStream_t s2 = (c->tun.icp_lowprio || (wg_of[1] > 0 && wg_of[2] > 0)) ? c->stream2 : c->stream;
    if (s1 != c->stream || s2 != c->stream) {   // everything uploaded so far is visible to the side streams
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        if (s1 != c->stream) HIPCHK(c, hipStreamWaitEvent(s1, c->ev2[0], 0));
        if (s2 != c->stream) HIPCHK(c, hipStreamWaitEvent(s2, c->ev2[0], 0));
    }
    if (wg_of[1] > 0) LAUNCH(c, launch_icp_pipe(s1, ncl, a.dev, a.tpl, a.scr, wg_of[1], c->d_wgtab + gl.tab_of[1], ipg, icp_bound(c)));
    if (wg_of[2] > 0) LAUNCH(c, launch_icp_pipe_big(s2, ncl, a.dev, a.tpl, a.scr, wg_of[2], c->d_wgtab + gl.tab_of[2], ipg, icp_bound(c)));
    if (s1 != c->stream && wg_of[1] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[2], s1));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[2], 0));
    }
    if (s2 != c->stream && wg_of[2] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[1], s2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[1], 0));
    }
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (ipg.pipe_slots << 16) | gl.n_wg;
    if (pl.nwork > 0) {   // the other clusters take the sliced driver
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    if (int e = icp_read_back(c, ncl)) return e;
    *done = true;
    return CD_OK;
}

// One launch in which every cluster runs its whole ICP in one workgroup (plan.whole_cluster): k_icp_pipe, k_icp_pipe_big or
// k_icp_cluster.  Always finishes the stage.
int icp_run_whole(cd_context* c, const IcpPlan& pl, const IcpArgs& a, IcpParams ip, bool* done) {
    const int ncl = pl.ncl, wg_cap = pl.wg_cap;
    const int grid = whole_launch_grid(ncl, wg_cap, c->tun.icp_cpw, pl.crowded, ip.pipe_slots);   // workgroups of the pipelined launches
    GateHold hold;   // (released on every path out of this function)
    if (c->tun.icp_concurrent > 0) hold.enter(&device_shared(c).icp_gate, c->tun.icp_concurrent);
    for (int k = 0; k < ncl; ++k) c->h_order[k] = k;
    largest_first(c->h_order, ncl, c->h_cl);
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * ncl, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int), c->stream));   // head of the cluster queue
    hipStream_t si = c->tun.icp_lowprio >= 2 ? c->stream3 : c->stream;
    if (pl.pipe_ok || pl.big_ok) {
        c->timing.icp_regime = (ip.pipe_slots << 16) | grid;
        ip.donate = whole_donate(c->tun.icp_donate, device_shared(c).batches_in_flight.load(), ncl, grid) ? 1 : 0;
        if (ip.donate) HIPCHK(c, hipMemsetAsync(c->d_don, 0, sizeof(int) * (size_t)(DON_BOX + DON_CAP), c->stream));
    }
    if (si != c->stream) {   // (after the control block was zeroed on c->stream: the launch on `si` must see it zeroed - ADVICE r4)
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        HIPCHK(c, hipStreamWaitEvent(si, c->ev2[0], 0));
    }
    if (pl.pipe_ok) LAUNCH(c, launch_icp_pipe(si, ncl, a.dev, a.tpl, a.scr, grid, nullptr, ip, icp_bound(c)));
    else if (pl.big_ok) LAUNCH(c, launch_icp_pipe_big(si, ncl, a.dev, a.tpl, a.scr, grid, nullptr, ip, icp_bound(c)));
    else LAUNCH(c, launch_icp_cluster(si, ncl, a.dev, a.tpl, a.scr, wg_cap, ip, icp_bound(c)));
    if (si != c->stream) {
        HIPCHK(c, hipEventRecord(c->ev2[2], si));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[2], 0));
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    c->timing.icp_kernel_launches = 1;
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    if (ip.donate) HIPCHK(c, xfer(c, c->h_ctl + 8, c->d_don, sizeof(int) * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;   // (also when the hand-over check below fails the call: icp_kernel_ms is reported)
    if (ip.donate) {
        const int* w = c->h_ctl + 8;   // (copied with the records above)
        c->timing.icp_handovers = w[DON_HEAD];
        // every cluster of the launch was finished by somebody, and every mailbox entry that was written was taken
        if (w[DON_ERR] != 0 || w[DON_FINISHED] != ncl || w[DON_HEAD] != std::min(w[DON_TAIL], DON_CAP)) {
            c->timing.icp_handover_lost = 1;
            std::snprintf(c->err, sizeof(c->err), "ICP hand-over lost a cluster: %d of %d clusters finished, %d entries published, %d taken, error word %d",
                          w[DON_FINISHED], ncl, w[DON_TAIL], w[DON_HEAD], w[DON_ERR]);
            return CD_ERR_DEVICE;
        }
        if (std::getenv("CUBOID_DEBUG"))
            std::fprintf(stderr, "cuboid_hip: hand-overs: %d published, %d taken, %d clusters finished of %d, waiting balance %d\n", w[DON_TAIL], w[DON_HEAD], w[DON_FINISHED], ncl, w[DON_AVAIL]);
    }
    return CD_OK;
}

// Few clusters: ONE persistent launch runs every iteration and the fitness pass (k_icp_persist: grid barrier per
// iteration instead of two kernel launches; when: persist_launch).  Needs all its workgroups resident together; a barrier that
// does not complete in time makes it give up, and the sliced driver takes over from the initial state (not done).
int icp_run_persist(cd_context* c, const IcpPlan& pl, const IcpArgs& a, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, nwork = pl.nwork;
    const PersistLaunch pe = persist_launch(c->h_cl, ncl, nwork, pl.wg_cap, c->tun.icp_persist, device_shared(c).calls_in_flight.load());
    if (!pe.launch) return CD_OK;
    // d_queue[4] barrier counter, [5] abort flag, [6..9] clusters closed per iteration slot (k_icp_persist's exit test)
    int* ctl = c->h_ctl;
    for (int i = 0; i < 8; ++i) ctl[i] = 0;
    ctl[1] = c->tun.icp_persist == 2 ? 1 : 0;
    HIPCHK(c, xfer(c, c->d_queue + 4, ctl, sizeof(int) * 6, hipMemcpyHostToDevice));
    LAUNCH(c, launch_icp_persist(c->stream, nwork, pe.G, ip.max_iter + 3, c->d_work, a.dev, a.tpl, a.scr, pl.qslice, (unsigned*)(c->d_queue + 4), c->d_queue + 5, pe.n_open,
                                 c->d_queue + 6, ip, icp_bound(c)));
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, xfer(c, ctl + 8, c->d_queue + 5, sizeof(int), hipMemcpyDeviceToHost));
    c->st_init.assign(c->h_st.get(), c->h_st + 2 * (size_t)ncl);   // in case the launch gives up (no reallocation after the first call)
    if (int e = icp_read_back(c, ncl)) return e;
    if (!ctl[8]) {   // (the abort flag: raised when the launch gave up)
        c->timing.icp_kernel_launches = 1;
        *done = true;
        return CD_OK;
    }
    c->persist_gave_up += 1;
    c->timing.icp_persist_gave_up += 1;
    if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: persistent ICP launch gave up at a grid barrier, running the multi-launch loop\n");
    // start over: initial states, zero sums, the source points as extracted (the launch transformed them in place)
    std::memcpy(c->h_st, c->st_init.data(), sizeof(IcpState) * 2 * (size_t)ncl);
    HIPCHK(c, xfer(c, c->d_st, c->h_st, sizeof(IcpState) * 2 * ncl, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, sizeof(unsigned long long) * 48 * (size_t)ncl, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_accf, 0, sizeof(unsigned long long) * (size_t)ncl, c->stream));
    if (c->icp_bounded) HIPCHK(c, hipMemsetAsync(c->d_ncorr, 0, sizeof(uint32_t) * 3 * (size_t)ncl, c->stream));
    long long span = 0;
    for (int k = 0; k < ncl; ++k) span = std::max(span, (long long)c->h_cl[k].src_off + c->h_cl[k].n);
    HIPCHK(c, hipMemcpyAsync(c->d_src, c->d_src0, sizeof(float4) * (size_t)span, hipMemcpyDeviceToDevice, c->stream));
    if (pl.guess_mode == CD_GUESS_CLUSTER)   // (the states just uploaded start from the identity again)
        if (int e = launch_cluster_guesses(c, ncl)) return e;
    if (pl.device_guesses)
        if (int e = launch_coarse_handover(c, ncl)) return e;
    if (guess_indexing(pl) >= 0)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl.max_n, c->d_cl, c->d_guess, guess_indexing(pl), c->d_src0, c->d_src));
    return CD_OK;
}

// The multi-launch loop over the work list, then the fitness pass.  Always finishes the stage.
// Rule C19 (cd_set_icp_median_rejection, plan.reject - every live cluster has items then): k_icp_reject behind every iteration
// launch: k_icp_solve<true>(it), k_icp_iter<true>(it), whose sums for the slot k_icp_reject(it) then replaces with those of the kept
// correspondences.  Always the BOUNDED instantiations then, with d2_max = +inf when rule C8 bounds nothing.
// Rule C22 (cd_set_icp_reciprocal, plan.recip): the same with k_icp_recip's two kernels in k_icp_reject's place; between them they
// hand one flag per source point through d_rkeep.
int icp_run_sliced(cd_context* c, const IcpPlan& pl, const IcpArgs& a, const IcpParams& ip, bool* done) {
    static_assert(sizeof(RejectStats) == sizeof(cd_icp_reject_stats), "RejectStats mirrors cd_icp_reject_stats");
    static_assert(sizeof(RecipStats) == sizeof(cd_icp_recip_stats), "RecipStats mirrors cd_icp_recip_stats");
    const int ncl = pl.ncl, nwork = pl.nwork, max_launch = ip.max_iter + 3;
    IcpBound bnd = icp_bound(c);
    if (pl.reject) {
        GROW(c, d_rstat, (size_t)ncl); GROW(c, h_rstat, (size_t)ncl);
        HIPCHK(c, hipMemsetAsync(c->d_rstat, 0, sizeof(RejectStats) * (size_t)ncl, c->stream));   // (pre-marked problems keep zeros)
    }
    int recip_max_n = 0;
    if (pl.recip) {   // the flags cover the live problems' points as d_src holds them
        long long span = 0;
        for (int k = 0; k < ncl; ++k) {
            if (c->h_cl[k].n < 3 || c->h_cl[k].tpl_m <= 0) continue;
            span = std::max(span, (long long)c->h_cl[k].src_off + c->h_cl[k].n);
            recip_max_n = std::max(recip_max_n, c->h_cl[k].n);
        }
        GROW(c, d_rkeep, (size_t)std::max(span, 1ll));
        GROW(c, d_qstat, (size_t)ncl); GROW(c, h_qstat, (size_t)ncl);
        HIPCHK(c, hipMemsetAsync(c->d_qstat, 0, sizeof(RecipStats) * (size_t)ncl, c->stream));   // (pre-marked problems keep zeros)
    }
    if (pl.filtered()) {
        if (!bnd.bounded) bnd.d2_max = std::numeric_limits<float>::infinity();
        bnd.bounded = 1;
    }
    // The iteration kernel walks an ACTIVE work list (d_work2) that the host re-packs at every
    // completion poll, dropping the clusters that have converged (repack_active); the full list (d_work) is kept for
    // the fitness pass (k_icp_solve alone keeps the state of a cluster without items).
    int it = 0, nactive = nwork;
    std::memcpy(c->h_work2, c->h_work, sizeof(IcpWork) * (size_t)std::max(nwork, 1));
    HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)std::max(nwork, 1), hipMemcpyHostToDevice));
    for (int polls = 0; nwork > 0 && it < max_launch; ++polls) {
        const int g = std::min(sliced_poll_group(polls), max_launch - it);
        for (int q = 0; q < g; ++q, ++it) {
            LAUNCH(c, launch_icp_iter(c->stream, it, nactive, ncl, c->d_work2, a.dev, a.tpl, a.scr, pl.qslice, c->n_cu, ip, bnd));
            if (pl.reject && nactive > 0) LAUNCH(c, launch_icp_reject(c->stream, it, ncl, a.dev, a.tpl, a.scr, bnd, c->reject_factor, c->d_rstat));
            if (pl.recip && nactive > 0) LAUNCH(c, launch_icp_recip(c->stream, it, ncl, recip_max_n, a.dev, a.tpl, a.scr, bnd, c->d_rkeep, c->d_qstat));
        }
        HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool all = false;
        const int na = repack_active(c->h_work, nwork, c->h_st, ncl, c->h_work2, &all);
        if (all) break;
        if (na != nactive) {
            nactive = na;
            if (na > 0) HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)na, hipMemcpyHostToDevice));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));   // (before the fitness pass)
    c->timing.icp_kernel_launches = it;               // (iteration launches)
    LAUNCH(c, launch_icp_fitness(c->stream, nwork, c->d_work, a.dev, 0, a.tpl, a.scr, pl.qslice));
    if (pl.reject) HIPCHK(c, xfer(c, c->h_rstat, c->d_rstat, sizeof(RejectStats) * (size_t)ncl, hipMemcpyDeviceToHost));
    if (pl.recip) HIPCHK(c, xfer(c, c->h_qstat, c->d_qstat, sizeof(RecipStats) * (size_t)ncl, hipMemcpyDeviceToHost));
    if (int e = icp_read_back(c, ncl)) return e;
    *done = true;
    return CD_OK;
}

}  // namespace

namespace cd {
// S6.  clusters described by h_cl[0..ncl) (src_off relative to d_src/d_src0).  Fills h_st / h_accf.  device_guesses: the fine
// stage of rule C18 - its set-up runs the hand-over from the tables stage_icp_levels has put on the stream.
int stage_icp(cd_context* c, int ncl, const cd_params* p, long long* pair_tests, bool device_guesses) {
    c->timing.icp_kernel_launches = 0;
    c->timing.icp_kernel_ms = 0.f;
    if (pair_tests) *pair_tests = 0;
    if (ncl <= 0) return CD_OK;
    IcpPlan pl;
    int st = plan_stage(c, ncl, p, device_guesses, &pl);
    if (!st) st = icp_setup(c, p, &pl);
    if (st) return st;
    const IcpParams ip = icp_params(c, p, &pl.crowded);
    const IcpArgs a = icp_args(c);
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    bool done = false;
    if (pl.plane) st = icp_run_plane(c, pl, a, ip, &done);
    if (!st && !done && pl.n_lat > 0) st = icp_run_lat(c, pl, a, ip, &done);
    if (!st && !done && pl.grouped_pipe) st = icp_run_grouped(c, pl, a, ip, &done);
    if (!st && !done && pl.whole_cluster) st = icp_run_whole(c, pl, a, ip, &done);
    if (!st && !done && !pl.filtered()) st = icp_run_persist(c, pl, a, ip, &done);   // (rules C19, C22: the sliced loop, nothing before it)
    if (!st && !done) st = icp_run_sliced(c, pl, a, ip, &done);
    if (done) icp_finish(c, ncl, pair_tests);
    return st;
}

// Rule C18.  Both levels are ordinary stages: the coarse one over the subsamples gathered behind the stage's
// clusters, then - its states, fitness sums and the hand-over table on the stream - the stage itself with per-problem guesses.
// stage_icp fills h_cl / h_st / h_accf from index 0, so what the coarse stage left there is copied out before the fine stage
// starts, and the stage's own problem list is kept aside meanwhile.  No device or pinned pointer is held across a stage.
int stage_icp_levels(cd_context* c, int ncl, const cd_params* p, long long* pair_tests) {
    if (c->coarse_stride == 0 || ncl <= 0) return stage_icp(c, ncl, p, pair_tests);
    const size_t cap = std::min(std::min(c->d_src0.capacity(), c->d_src.capacity()), std::min(c->d_nn.capacity(), c->d_d2.capacity()));
    CoarsePlan cp;
    if (plan_coarse(c->h_cl, ncl, c->coarse_stride, c->coarse_min, (long long)cap, &cp) != CD_OK)
        return fail(c, CD_ERR_CAPACITY, "coarse-to-fine ICP: the coarse sets do not fit behind the stage's clusters in the ICP source buffers");
    GROW(c, h_cstat, (size_t)ncl);
    if (cp.n_eligible == 0) {   // an ordinary stage, stream operation for stream operation; its stats say "not eligible"
        std::memset(c->h_cstat.get(), 0, sizeof(CoarseStats) * (size_t)ncl);
        return stage_icp(c, ncl, p, pair_tests);
    }
    const int nc = cp.n_eligible;
    GROW(c, d_cstat, (size_t)ncl); GROW(c, d_chand, (size_t)ncl); GROW(c, h_chand, (size_t)ncl);
    GROW(c, d_cgather, (size_t)nc); GROW(c, h_cgather, (size_t)nc);
    GROW(c, d_cst, (size_t)nc); GROW(c, h_cst, (size_t)nc); GROW(c, d_caccf, (size_t)nc); GROW(c, h_caccf, (size_t)nc);
    const std::vector<IcpCluster> fine(c->h_cl.get(), c->h_cl.get() + ncl);
    // the coarse level
    std::memcpy(c->h_cgather.get(), cp.gather.data(), sizeof(CoarseGather) * (size_t)nc);
    HIPCHK(c, xfer(c, c->d_cgather, c->h_cgather, sizeof(CoarseGather) * (size_t)nc, hipMemcpyHostToDevice));
    LAUNCH(c, launch_icp_coarse_gather(c->stream, nc, cp.max_n_coarse, c->d_cgather, c->d_src0, c->d_src));
    std::memcpy(c->h_cl.get(), cp.coarse.data(), sizeof(IcpCluster) * (size_t)nc);
    long long pairs_c = 0;
    // (icp_wave_ms is written by the lattice driver only and stage_icp leaves it alone otherwise: each level's own value is read
    // from zero, and what was there stays when neither level writes it)
    const float wave_before = c->timing.icp_wave_ms;
    c->timing.icp_wave_ms = 0.f;
    int st = stage_icp(c, nc, p, &pairs_c);   // (ends synchronised)
    const int launches_c = c->timing.icp_kernel_launches;
    const float ms_c = c->timing.icp_kernel_ms, wave_c = c->timing.icp_wave_ms;
    c->timing.icp_wave_ms = st ? wave_before : 0.f;
    for (int j = 0; j < nc && !st; ++j) { c->h_cst[j] = c->h_st[2 * j]; c->h_caccf[j] = c->h_accf[j]; }
    std::memcpy(c->h_cl.get(), fine.data(), sizeof(IcpCluster) * (size_t)ncl);
    if (st) return st;
    // the hand-over and the fine level
    std::memcpy(c->h_chand.get(), cp.hand.data(), sizeof(CoarseHand) * (size_t)ncl);
    {
        XferBatch xb(c);   // (one launch)
        xb.add(c->d_cst, c->h_cst, sizeof(IcpState) * (size_t)nc, hipMemcpyHostToDevice);
        xb.add(c->d_caccf, c->h_caccf, sizeof(unsigned long long) * (size_t)nc, hipMemcpyHostToDevice);
        xb.add(c->d_chand, c->h_chand, sizeof(CoarseHand) * (size_t)ncl, hipMemcpyHostToDevice);
        HIPCHK(c, xb.flush());
    }
    st = stage_icp(c, ncl, p, pair_tests, /*device_guesses=*/true);
    if (st) return st;
    c->timing.icp_kernel_launches += launches_c + 2;   // (the gather and the hand-over)
    c->timing.icp_kernel_ms += ms_c;
    const float wave = wave_c + c->timing.icp_wave_ms;
    c->timing.icp_wave_ms = wave > 0.f ? wave : wave_before;
    if (pair_tests) *pair_tests += pairs_c;
    return CD_OK;
}

void fill_cluster_result(const cd_context* c, int k, const cd_params* p, cd_cluster_result* r) {
    const IcpState& st = c->h_st[2 * k];
    const IcpCluster& cl = c->h_cl[k];
    std::memset(r, 0, sizeof(*r));
    r->size = cl.n;
    r->iterations = st.iters;
    r->converged = st.converged;
    std::memcpy(r->T, st.Tfinal, 64);
    r->fitness = st.status == CD_OK ? hm::unfix(c->h_accf[k], FIX_SHIFT_D2) / (double)cl.n : std::numeric_limits<double>::max();
    r->accepted = (r->converged && r->fitness < p->icp_accept_fitness) ? 1 : 0;
    double Td[16];
    for (int i = 0; i < 16; ++i) Td[i] = (double)st.Tfinal[i];
    if (!hm::mat4_inverse(Td, r->pose))
        for (int i = 0; i < 16; ++i) r->pose[i] = std::numeric_limits<double>::quiet_NaN();
}
}  // namespace cd
