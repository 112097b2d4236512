// batch.hip - the fused batch call: its steps, process_batch_impl, the cd_process_* entry points (point records and depth
// images) and the read-backs of the last call's results.
#include "context.hpp"

namespace {
// what a fused call's gate needs besides cd_params, checked before anything is copied or launched: `color` = the call is a
// depth call with registered colour images
int check_bbox_source(cd_context* c, const cd_params* p, int F, bool color) {
    if (!p || !p->bbox_enable || c->bbox_source == CD_BBOX_PARAMS) return CD_OK;
    if (c->bbox_source == CD_BBOX_PER_FRAME) {
        if (F > 0 && c->frame_rects.size() < 4 * (size_t)F) return fail(c, CD_ERR_INVALID_ARG, "bbox source CD_BBOX_PER_FRAME but cd_set_frame_bboxes holds fewer rectangles than the batch has frames");
        return CD_OK;
    }
    if (!color) return fail(c, CD_ERR_INVALID_ARG, "bbox source CD_BBOX_COLOR needs cd_process_depth_batch[_device] with CD_COLOR_RGB8 images");
    return CD_OK;
}

// ---- the fused batch call ---------------------------------------------------------------------------------------
// process_batch_impl, at the end of this section, is the sequence; the functions before it are its steps in the order it calls
// them.  Each says what it issues on the context's stream and which synchronisation it relies on.

// What a fused call sets on the context for its own duration only, put back on every way out: the rectangles its gate kernels
// read (call_rects) and the two marks of the zero launch that make the stages skip their own fills (batch_zeroed, fs_initialised).
struct BatchScope {
    cd_context* c;
    ~BatchScope() { c->call_rects = FrameRects{nullptr, 0}; c->batch_zeroed = false; c->fs_initialised = false; }
};

// Every scratch array the stages want zeroed, in ONE launch (a batch had ~14 fill kernels, each a stream operation of its own
// that queues behind the other contexts' kernels).  A scratch array that a stage expects zeroed is added to THIS list.
// Issues that launch and sets batch_zeroed / fs_initialised (BatchScope puts them back); relies on no synchronisation.
int zero_batch_scratch(cd_context* c, int F) {
    ZeroRegions zr;
    zr.n = 0;
    zr.fs = c->tun.mirror_writes && c->tun.copy_kernels ? c->d_fs : nullptr;   // (the crop stage then skips its upload of the initial FrameStates)
    zr.nfs = F;
    c->fs_initialised = zr.fs != nullptr;
    auto add = [&](void* ptr, size_t bytes) { zr.ptr[zr.n] = (uint32_t*)ptr; zr.words[zr.n] = bytes / 4; ++zr.n; };
    const size_t FT = (size_t)F * c->T;
    add(c->d_ticket, sizeof(int) * (size_t)F * TICKET_PITCH);
    add(c->d_tileA, sizeof(int) * FT);
    add(c->d_tileB, sizeof(int) * FT);
    add(c->d_tileC, sizeof(int) * FT);
    add(c->d_tile64, sizeof(unsigned long long) * FT);
    add(c->d_ghist, sizeof(uint32_t) * (size_t)F * SORT_MAX_PASSES_HOST * RADIX);
    add(c->d_counts, sizeof(int) * (size_t)F * MAX_HYP);
    add(c->d_sums, sizeof(unsigned long long) * 10 * (size_t)F);
    add(c->d_tileK, sizeof(int) * FT * KICP);
    add(c->d_acc, sizeof(unsigned long long) * 48 * (size_t)c->cl_cap);
    add(c->d_accf, sizeof(unsigned long long) * ((size_t)c->cl_cap + 1));
    add(c->d_queue, sizeof(int) * 16);
    LAUNCH(c, launch_zero_regions(c->stream, zr));
    c->batch_zeroed = true;
    return CD_OK;
}

// The call's stream work ahead of the crop stage, all of it after ev[0] and so inside stage [0] of the timing: the gate's
// per-frame rectangles (an upload for CD_BBOX_PER_FRAME, the colour stage for CD_BBOX_COLOR, whose records feed the gate on
// the device; call_rects then points at them), the deprojection of a depth call into d_frames, and the zero launch.
// Relies on no synchronisation and makes none.
int batch_prologue(cd_context* c, int gate_source, const void* d_frames, int F, const DepthJob* dj) {
    if (gate_source == CD_BBOX_PER_FRAME) {
        std::memcpy(c->h_rects, c->frame_rects.data(), sizeof(int32_t) * 4 * (size_t)F);
        HIPCHK(c, xfer(c, c->d_rects, c->h_rects, sizeof(int32_t) * 4 * (size_t)F, hipMemcpyHostToDevice));
        c->call_rects = FrameRects{c->d_rects, 4};
    } else if (gate_source == CD_BBOX_COLOR) {
        // (a mapped call: the raw colour images at their own size, so the rectangles are in colour pixels)
        int st = stage_color(c, dj->color, dj->ccam ? dj->ccam->width : dj->cam->width, dj->ccam ? dj->ccam->height : dj->cam->height, F, &c->color_prm);
        if (st) return st;
        c->call_rects = FrameRects{reinterpret_cast<const int32_t*>(c->d_crec.get()), (int32_t)(sizeof(ColorRecord) / sizeof(int32_t))};   // (rect is the record's first member)
    }
    if (dj) LAUNCH(c, launch_depth_job(c->stream, dj, F, (float4*)const_cast<void*>(d_frames)));
    return c->tun.zero_once ? zero_batch_scratch(c, F) : CD_OK;
}

struct FrontStages {   // what the front stages leave for the frame records
    std::vector<int> iterations;     // RANSAC iterations of every frame (stage_plane)
    int rounds = 0;                  // hypothesis rounds of the plane stage
    std::vector<char> gave_up;       // the frames whose sampler ran into a device limit (stage_plane; the surface fits run it again)
    std::vector<char> surface_flag;  // CD_GUESS_SURFACE: the frames whose guess came from their surface fit (empty otherwise)
};

struct BatchClusters {   // the host's table of a batch's clusters, frame-major (batch_clusters)
    std::vector<int> first;       // index of frame f's first cluster (F + 1 entries)
    std::vector<int> size, off;   // per cluster: its points; where its ICP source starts in the frame's segment of d_src0 / d_src
    std::vector<int> span;        // per frame: the points of all its clusters, i.e. of one copy of its ICP sources
    int ncl = 0, kmax = 0;        // clusters of the batch; of its fullest frame
    int rounds_k = 1;             // extraction rounds: ceil(kmax / KICP)
    long long points = 0;         // points of all clusters
    int To = 1;                   // tiles of the frame with the most object points (grid of the label kernels)
};

// Every cluster of every frame gets its ICP (opd.cpp:376-413).  The device extracts the ICP sources KICP clusters per frame at a
// time; frames with more than KICP clusters (rare) need further rounds, and the host needs their sizes.
// Fills the table from h_fs as stage_cluster_sync's synchronisation left it.  For each frame beyond KICP it issues one D2H copy
// of the sizes from d_sizes straight into cl->size and then synchronises the stream: cl->size is sized before the first copy and
// neither resized nor read until that synchronisation.  Ends with ensure_clusters for one ICP problem per cluster.
int batch_clusters(cd_context* c, int F, BatchClusters* cl) {
    cl->first.assign((size_t)F + 1, 0);
    int max_no = 0;   // (read again after the cluster stage's own synchronisation, not handed down from before it)
    for (int f = 0; f < F; ++f) {
        cl->first[(size_t)f] = cl->ncl;
        cl->ncl += c->h_fs[f].n_k;
        cl->kmax = std::max(cl->kmax, c->h_fs[f].n_k);
        max_no = std::max(max_no, c->h_fs[f].n_o);
    }
    cl->first[(size_t)F] = cl->ncl;
    cl->To = std::max(1, (max_no + TILE - 1) / TILE);
    cl->rounds_k = std::max(1, (cl->kmax + KICP - 1) / KICP);
    cl->size.assign((size_t)std::max(cl->ncl, 1), 0);
    cl->off.assign((size_t)std::max(cl->ncl, 1), 0);
    for (int f = 0; f < F; ++f) {
        const FrameState& s = c->h_fs[f];
        int* sz = cl->size.data() + cl->first[(size_t)f];
        if (s.n_k > KICP) HIPCHK(c, hipMemcpyAsync(sz, c->d_sizes + (size_t)f * c->N, sizeof(int) * (size_t)s.n_k, hipMemcpyDeviceToHost, c->stream));
        else for (int k = 0; k < s.n_k; ++k) sz[k] = s.ksize[k];
    }
    if (cl->rounds_k > 1) HIPCHK(c, hipStreamSynchronize(c->stream));
    cl->span.assign((size_t)F, 0);
    for (int f = 0; f < F; ++f) {
        int off = 0;
        for (int k = cl->first[(size_t)f]; k < cl->first[(size_t)f + 1]; ++k) { cl->off[(size_t)k] = off; off += cl->size[(size_t)k]; }
        cl->span[(size_t)f] = off;
        cl->points += off;
    }
    return ensure_clusters(c, cl->ncl, cl->points);
}

// d_koffx: the offsets the label scatter writes the ICP sources to, [copy][round][F][KICP].  Cluster q of frame f starts, in
// copy t, at off[q] + t * span[f] of the frame's segment.  copies == 1 is the table of the per-template passes; they pass
// nullptr (packed) for round 0, so its round-0 words are never read.
// Grows d_koffx (which synchronises the stream when it has to) and uploads the table with a blocking copy.
int upload_koffx(cd_context* c, int F, const BatchClusters& cl, int copies) {
    const size_t need = (size_t)copies * cl.rounds_k * F * KICP;
    GROW(c, d_koffx, need);
    std::vector<int> tab(need, 0);
    for (int t = 0; t < copies; ++t)
        for (int r = 0; r < cl.rounds_k; ++r)
            for (int f = 0; f < F; ++f)
                for (int k = 0; k < KICP; ++k) {
                    const int q = cl.first[(size_t)f] + r * KICP + k;
                    if (q < cl.first[(size_t)f + 1]) tab[(((size_t)t * cl.rounds_k + r) * F + f) * KICP + k] = cl.off[(size_t)q] + t * cl.span[(size_t)f];
                }
    HIPCHK(c, copy_sync(c, c->d_koffx, tab.data(), sizeof(int) * need, hipMemcpyHostToDevice));
    return CD_OK;
}
const int* koffx_at(const cd_context* c, int F, const BatchClusters& cl, int t, int r) { return c->d_koffx + (((size_t)t * cl.rounds_k + r) * F) * KICP; }

// Extraction round r of the ICP sources: the clusters ranked [r * KICP, (r + 1) * KICP) of every frame, to the offsets koff
// ([F][KICP]; nullptr: packed, round 0 only).  With a single round the tile counts of stage_cluster are still in d_tileK.
// Issues the label scatter, behind a memset, a count and a scan of d_tileK when there are several rounds; no synchronisation.
int extract_round(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, int r, const int* koff) {
    if (cl.rounds_k > 1) {
        HIPCHK(c, hipMemsetAsync(c->d_tileK, 0, sizeof(int) * (size_t)F * KICP * c->T, c->stream));
        LAUNCH(c, launch_label_count(c->stream, c->N, F, c->T, cl.To, c->d_fs, p->cluster_enable, c->d_parent, c->d_rank, c->d_label, c->d_tileK, r * KICP));
        LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileK, F * KICP, c->T, nullptr, 0));
    }
    LAUNCH(c, launch_label_scatter(c->stream, c->d_obj, c->N, F, c->T, cl.To, c->d_fs, c->d_label, c->d_tileK, c->d_src0, c->d_src, r * KICP, koff));
    return CD_OK;
}

// (Re)builds the ICP sources d_src0 / d_src of every round (upload_koffx with one copy has run when there are several).
// Round 0 was extracted by stage_cluster; it is redone only when d_src has been consumed by a previous template pass or
// d_tileK by a later round.
int extract_sources(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, bool redo_round0) {
    for (int r = redo_round0 ? 0 : 1; r < cl.rounds_k; ++r)
        if (int e = extract_round(c, p, F, cl, r, r > 0 ? koffx_at(c, F, cl, 0, r) : nullptr)) return e;
    return CD_OK;
}

// The opt-in ICP steps that keep one record per cluster: fn(the step is on, its kept table, the pinned mirror of a stage's records).
// A new step adds its line here.
template <class Fn>
void for_each_icp_stat(cd_context* c, Fn&& fn) {
    fn(c->plane_weight != 0.0, c->last_plane, c->h_pstat);     // rule C17
    fn(c->coarse_stride != 0, c->last_coarse, c->h_cstat);     // rule C18
    fn(c->reject_factor != 0.0, c->last_reject, c->h_rstat);   // rule C19
    fn(c->recip_on != 0, c->last_recip, c->h_qstat);           // rule C22
}

struct BatchIcp {   // the ICP part of a fused call; the results themselves are kept in c->last_clusters
    std::vector<int> slots;                    // the template slots every cluster is matched against, ascending
    std::vector<long long> orig_off, al_off;   // per cluster, see cd_get_cluster_points (publish_last hands them to the context)
    long long pairs = 0;                       // pair tests of all its stages
};

// The first statement of the ICP part: the per-cluster results of the previous batch go away.  last_first stays empty until
// publish_last, so a failure in between leaves cd_get_cluster_results with "no batch" rather than old offsets into new results.
// template_slot >= 0: every cluster against that slot; -1: against every loaded template.  Host only.
void begin_batch_icp(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    c->last_first.clear();
    if (p->template_slot >= 0) bi->slots.push_back(p->template_slot);
    else for (int sidx = 0; sidx < CD_MAX_TEMPLATES; ++sidx) if (c->tpl_m[sidx] > 0) bi->slots.push_back(sidx);
    if (bi->slots.empty()) bi->slots.push_back(0);
    c->last_clusters.assign((size_t)std::max(cl.ncl, 1), cd_cluster_result());
    bi->orig_off.assign((size_t)std::max(cl.ncl, 1), -1);
    bi->al_off.assign((size_t)std::max(cl.ncl, 1), -1);
    for_each_icp_stat(c, [&](bool on, auto& kept, auto&) { if (on) kept.begin(cl.ncl); });   // the kept result's record, not valid before publish_last
    for (int f = 0; f < F; ++f)
        for (int q = cl.first[(size_t)f]; q < cl.first[(size_t)f + 1]; ++q) bi->orig_off[(size_t)q] = (long long)f * c->N + cl.off[(size_t)q];
}

// Several templates: when S copies of every frame's ICP sources fit its segment of the source buffers (they do unless a frame
// is nearly all objects), every (cluster, template) pair becomes one ICP problem of ONE stage - the batch then fills the chip
// with S x ncl problems instead of running S under-filled passes one after the other.
bool fits_one_stage(const cd_context* c, int F, const BatchClusters& cl, int S) {
    if (S <= 1 || cl.ncl <= 0 || (long long)S * cl.ncl > 0x3fffffffll) return false;
    for (int f = 0; f < F; ++f)
        if ((long long)S * cl.span[(size_t)f] > (long long)c->N) return false;
    return true;
}

// ICP problem q of the stage just run (synchronised by stage_icp) is cluster k against `slot`.  Its result is kept when it
// is the cluster's first or has the lower fitness, so - the slots ascending - ties keep the lowest slot.  `resident`: the
// problem's aligned points are still in d_src when the call returns (al_off; -1 otherwise).
void keep_lower_fitness(cd_context* c, const cd_params* p, BatchIcp* bi, int q, int k, int slot, bool first, bool resident) {
    cd_cluster_result r;
    fill_cluster_result(c, q, p, &r);
    r.template_slot = slot;
    if (!first && !(r.fitness < c->last_clusters[(size_t)k].fitness)) return;
    c->last_clusters[(size_t)k] = r;
    for_each_icp_stat(c, [&](bool on, auto& kept, auto& mirror) { if (on) kept.keep(k, mirror[q]); });
    bi->al_off[(size_t)k] = resident ? (long long)c->h_cl[q].src_off : -1;
}

// CD_GUESS_CLUSTER: the records of the stage just run (h_shape, on the host since stage_icp's synchronisation) for
// cd_get_cluster_shape_frames - problem k < ncl is cluster k.
void keep_cluster_shapes(cd_context* c, const cd_params* p, int ncl) {
    if (p->icp_use_guess != CD_GUESS_CLUSTER) return;
    c->last_shapes.assign_all(c->h_shape.get(), ncl);
}

// All (cluster, template) pairs in one stage (fits_one_stage): problem t * ncl + k is cluster k against slots[t], on copy t of
// the sources.  Uploads the offset table of S copies, issues every extraction round of every copy and one stage_icp, which
// ends synchronised.  Every problem's aligned points stay resident.
int icp_all_pairs(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    const int S = (int)bi->slots.size(), ncl = cl.ncl;
    int st = upload_koffx(c, F, cl, S);
    if (st) return st;
    for (int t = 0; t < S; ++t)
        for (int r = 0; r < cl.rounds_k; ++r) {
            st = extract_round(c, p, F, cl, r, koffx_at(c, F, cl, t, r));
            if (st) return st;
        }
    st = ensure_clusters(c, S * ncl, (long long)S * cl.points);
    if (st) return st;
    for (int t = 0; t < S; ++t)
        for (int f = 0; f < F; ++f) {
            const int q = cl.first[(size_t)f];
            set_icp_clusters(c, t * ncl + q, c->h_fs[f].n_k, f, cl.size.data() + q, cl.off.data() + q, f * c->N + t * cl.span[(size_t)f], bi->slots[(size_t)t]);
        }
    st = stage_icp_levels(c, S * ncl, p, &bi->pairs);
    if (st) return st;
    keep_cluster_shapes(c, p, ncl);   // (the problems of slots[0]: a cluster's record does not depend on the template)
    for (int t = 0; t < S; ++t)
        for (int k = 0; k < ncl; ++k) keep_lower_fitness(c, p, bi, t * ncl + k, k, bi->slots[(size_t)t], t == 0, true);
    return CD_OK;
}

// One ICP pass per slot, every cluster against it.  The sources are re-extracted between passes (ICP transforms d_src in
// place), so the aligned cloud of a pass stays in d_src only until the next one: only the last slot's is resident.
// Uploads the later rounds' offsets when there are several rounds; per pass: extract_sources, then one stage_icp, which ends
// synchronised.
int icp_per_template(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    const int S = (int)bi->slots.size();
    if (cl.rounds_k > 1)
        if (int e = upload_koffx(c, F, cl, 1)) return e;
    for (int t = 0; t < S; ++t) {
        int st = extract_sources(c, p, F, cl, t > 0);
        if (st) return st;
        for (int f = 0; f < F; ++f) {
            const int q = cl.first[(size_t)f];
            set_icp_clusters(c, q, c->h_fs[f].n_k, f, cl.size.data() + q, cl.off.data() + q, f * c->N, bi->slots[(size_t)t]);
        }
        long long pr = 0;
        st = stage_icp_levels(c, cl.ncl, p, &pr);
        if (st) return st;
        keep_cluster_shapes(c, p, cl.ncl);
        bi->pairs += pr;
        for (int k = 0; k < cl.ncl; ++k) keep_lower_fitness(c, p, bi, k, k, bi->slots[(size_t)t], t == 0, t + 1 == S);
    }
    return CD_OK;
}

// The selection (cd_set_box_select) in a template_slot = -1 call: sel[k] >= 0 names the one slot cluster k is registered against
// (its box record matched it), -1 leaves it to every loaded slot.  One ICP pass per slot, as icp_per_template, over the clusters
// that take that slot: problem q of a pass is cluster prob[q], built exactly as the single-slot call builds it, so a selected
// cluster's result is that call's.  A slot nobody takes has no pass.  Only the last pass's aligned clouds stay resident.
int icp_selected(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi, const std::vector<int>& sel) {
    const int S = (int)bi->slots.size();
    if (cl.rounds_k > 1)
        if (int e = upload_koffx(c, F, cl, 1)) return e;
    std::vector<int> frame_of((size_t)cl.ncl, 0);
    for (int f = 0; f < F; ++f)
        for (int k = cl.first[(size_t)f]; k < cl.first[(size_t)f + 1]; ++k) frame_of[(size_t)k] = f;
    auto takes = [&](int k, int t) { return sel[(size_t)k] < 0 || sel[(size_t)k] == bi->slots[(size_t)t]; };
    int last_pass = -1;
    for (int t = 0; t < S; ++t)
        for (int k = 0; k < cl.ncl; ++k) if (takes(k, t)) { last_pass = t; break; }
    std::vector<char> seen((size_t)cl.ncl, 0);
    if (p->icp_use_guess == CD_GUESS_CLUSTER) c->last_shapes.begin(cl.ncl);
    bool first_pass = true;
    for (int t = 0; t <= last_pass; ++t) {
        std::vector<int> prob;
        for (int k = 0; k < cl.ncl; ++k) if (takes(k, t)) prob.push_back(k);
        if (prob.empty()) continue;
        int st = extract_sources(c, p, F, cl, !first_pass);
        if (st) return st;
        first_pass = false;
        const int slot = bi->slots[(size_t)t];
        for (size_t q = 0; q < prob.size(); ++q) {
            const int k = prob[q], f = frame_of[(size_t)k];
            c->h_cl[q] = IcpCluster{f * c->N + cl.off[(size_t)k], cl.size[(size_t)k], f, k - cl.first[(size_t)f], c->tpl_off[slot], c->tpl_m[slot], 0, slot};
        }
        long long pr = 0;
        st = stage_icp_levels(c, (int)prob.size(), p, &pr);
        if (st) return st;
        bi->pairs += pr;
        for (size_t q = 0; q < prob.size(); ++q) {
            const int k = prob[q];
            if (p->icp_use_guess == CD_GUESS_CLUSTER && !seen[(size_t)k]) c->last_shapes.keep(k, c->h_shape[q]);
            keep_lower_fitness(c, p, bi, (int)q, k, slot, !seen[(size_t)k], t == last_pass);
            seen[(size_t)k] = 1;
        }
    }
    return CD_OK;
}

// The state behind the read-back calls (cd_get_cluster_results, cd_get_cluster_points, cd_get_frame_cloud), published once
// every ICP stage of the batch has succeeded: the only place last_first is assigned.  Host only.
void publish_last(cd_context* c, const cd_params* p, int F, const BatchClusters& cl, BatchIcp* bi) {
    c->last_first = cl.first;
    c->last_orig_off.swap(bi->orig_off);
    c->last_al_off.swap(bi->al_off);
    c->last_nv.resize((size_t)F); c->last_no.resize((size_t)F);
    for (int f = 0; f < F; ++f) { c->last_nv[(size_t)f] = c->h_fs[f].n_v; c->last_no[(size_t)f] = c->h_fs[f].n_o; }
    c->last_clouds = true;
    c->last_surface_ok = p->icp_use_guess == CD_GUESS_SURFACE;
    if (p->icp_use_guess == CD_GUESS_CLUSTER) c->last_shapes.publish(cl.first);   // (keep_cluster_shapes has run, also for no cluster)
    for_each_icp_stat(c, [&](bool on, auto& kept, auto&) { if (on) kept.publish(cl.first); });
    if (c->pair_on) c->last_pair.publish(cl.first);   // rule C21 (stage_pair_scores has filled it)
    if (c->pose_on) c->last_pose.publish(cl.first);   // rule C23 (stage_pose_info has filled it)
    if (c->box_on) c->last_box.publish(cl.first);     // rule C24 (stage_box_fit has filled it)
}

// The per-frame records from h_fs, the plane mirrors and c->last_clusters, and the byte counts of the timing
// (algorithmic_bytes, icp_algorithmic_bytes).  Host only; every stage has been synchronised.
void write_frame_records(cd_context* c, int N, int F, const BatchClusters& cl, const FrontStages& fr, cd_frame_result* results) {
    static_assert(offsetof(ShapeFrame, mean) == offsetof(cd_shape_frame, mean) && offsetof(ShapeFrame, hi) == offsetof(cd_shape_frame, hi), "ShapeFrame mirrors cd_shape_frame");
    long long balg = 0;
    for (int f = 0; f < F; ++f) {
        const FrameState& s = c->h_fs[f];
        cd_frame_result& r = results[f];
        std::memset(&r, 0, sizeof(r));
        r.status = s.status;
        r.n_cropped = s.n_cropped;
        r.n_voxels = s.n_v;
        r.n_plane = s.n_plane;
        r.n_objects = s.n_o;
        r.n_clusters = s.n_k;
        r.flags = s.n_k > KICP ? CD_FRAME_MORE_CLUSTERS : 0;
        if (!fr.surface_flag.empty() && fr.surface_flag[(size_t)f]) r.flags |= CD_FRAME_SURFACE_GUESS;
        r.ransac_iterations = fr.iterations[f];
        if (s.status == CD_OK && !c->h_have[f]) r.status = fr.gave_up[(size_t)f] ? CD_ERR_CAPACITY : CD_ERR_NO_MODEL;
        if (c->h_have[f]) { r.plane[0] = c->h_model[f].x; r.plane[1] = c->h_model[f].y; r.plane[2] = c->h_model[f].z; r.plane[3] = c->h_model[f].w; }
        balg += 12ll * N + 12ll * s.n_v + 12ll * s.n_v * (fr.rounds + 3) + 4ll * s.n_v + 16ll * s.n_o + 200ll * s.n_k;
        for (int k = 0; k < s.n_k; ++k) {
            const cd_cluster_result& cr = c->last_clusters[(size_t)(cl.first[(size_t)f] + k)];
            if (k < KICP) r.clusters[k] = cr;
            if (c->last_shapes.valid()) {   // CD_GUESS_CLUSTER: did this cluster's ICP (against the template it kept) start from a rule-C13 guess?
                ShapeFrame rec;
                float G[16];
                std::memcpy(&rec, &c->last_shapes[(size_t)(cl.first[(size_t)f] + k)], sizeof(rec));
                if (shape_guess(rec, template_frame(c, cr.template_slot), G) >= 0) r.flags |= CD_FRAME_CLUSTER_GUESS;
            }
            const long long b = 12ll * c->tpl_m[cr.template_slot] + 12ll * cr.size * (cr.iterations + 1);
            balg += b;
            c->timing.icp_algorithmic_bytes += b;
        }
    }
    c->timing.algorithmic_bytes = balg;
}

// The optional plane_inliers / labels outputs ([F][N], -1 beyond a frame's count): one blocking D2H copy per frame and output.
int copy_frame_indices(cd_context* c, int N, int F, int32_t* plane_inliers, int32_t* labels) {
    for (int f = 0; f < F && (plane_inliers || labels); ++f) {
        const FrameState& s = c->h_fs[f];
        if (plane_inliers) {
            int32_t* dst = plane_inliers + (size_t)f * N;
            std::fill(dst, dst + N, -1);
            if (s.n_plane > 0) HIPCHK(c, copy_sync(c, dst, c->d_plane_idx + (size_t)f * c->N, sizeof(int) * s.n_plane, hipMemcpyDeviceToHost));
        }
        if (labels) {
            int32_t* dst = labels + (size_t)f * N;
            std::fill(dst, dst + N, -1);
            if (s.n_o > 0) HIPCHK(c, copy_sync(c, dst, c->d_label + (size_t)f * c->N, sizeof(int) * s.n_o, hipMemcpyDeviceToHost));
        }
    }
    return CD_OK;
}

// The stage times between the events ev[0..4] of process_batch_impl ([4]: the whole call) and the pair-test count.
// Waits for ev[4].
int read_stage_timing(cd_context* c, long long pairs) {
    HIPCHK(c, hipEventSynchronize(c->ev[4]));
    for (int k = 0; k < 4; ++k) hipEventElapsedTime(&c->timing.stage_ms[k], c->ev[k], c->ev[k + 1]);
    hipEventElapsedTime(&c->timing.stage_ms[4], c->ev[0], c->ev[4]);
    c->timing.icp_pair_tests_lo = (int32_t)(pairs & 0xffffffffll);
    c->timing.icp_pair_tests_hi = (int32_t)(pairs >> 32);
    return CD_OK;
}

// cd_get_frame_bboxes: the rectangles this call's gate used.  Host only; the colour records' mirrors (h_crec, h_cstatus) have
// been valid since the call's first synchronisation.
int publish_bboxes(cd_context* c, int gate_source, int F) {
    if (gate_source == CD_BBOX_PARAMS) return CD_OK;
    c->last_bboxes.assign((size_t)F, cd_color_bbox{});
    for (int f = 0; f < F; ++f) {
        if (gate_source == CD_BBOX_COLOR) std::memcpy(&c->last_bboxes[(size_t)f], &c->h_crec[f], sizeof(cd_color_bbox));
        else { std::memcpy(c->last_bboxes[(size_t)f].rect, c->frame_rects.data() + 4 * (size_t)f, sizeof(int32_t) * 4); c->last_bboxes[(size_t)f].found = 1; }
    }
    if (gate_source == CD_BBOX_COLOR)
        if (int st = color_status(c, F)) return st;
    c->last_bboxes_ok = true;
    return CD_OK;
}

// The fused call, in the order of DESIGN.md §5.  The event records ev[0..4] (the boundaries of cd_timing.stage_ms) and the
// release of the front gate are all here.
int process_batch_impl(cd_context* c, const void* d_frames, size_t stride, int N, int F, const cd_params* p,
                       cd_frame_result* results, int32_t* plane_inliers, int32_t* labels, const DepthJob* dj = nullptr) {
    // checks: nothing is copied or launched before they have passed
    int st = check_params(c, p);
    if (!st) st = check_bbox_source(c, p, F, dj && dj->color);
    if (!st) st = check_icp_modes(c, p->template_slot);   // rule C17: lattice templates only; rule C19: not together with rule C17
    if (st) return st;
    if (!results || !d_frames) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (N <= 0 || F <= 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad shape/stride");
    if (N > c->N || F > c->F) return fail(c, CD_ERR_CAPACITY, "batch larger than the context capacity");
    invalidate_last(c);
    std::memset(&c->timing, 0, sizeof(c->timing));
    InFlight in_flight(device_shared(c).batches_in_flight);
    GateHold front;
    if (c->tun.front_concurrent > 0) front.enter(&device_shared(c).front_gate, c->tun.front_concurrent);
    const int gate_source = p->bbox_enable ? c->bbox_source : CD_BBOX_PARAMS;
    BatchScope scope{c};
    // [0] gate rectangles, deprojection, zero launch, crop + voxel grid
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    st = batch_prologue(c, gate_source, d_frames, F, dj);
    if (!st) st = stage_crop_voxel(c, d_frames, stride, N, F, p, nullptr);
    if (!st) st = sync_fs(c, F);   // n_v
    if (st) return st;
    // [1] plane
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    FrontStages fr;
    st = stage_plane(c, F, p, fr.iterations, &fr.rounds);
    if (st) return st;
    fr.gave_up = c->plane_gave_up;
    // [2] extract, cluster, surface guesses
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    st = stage_extract(c, F, p);
    if (!st) st = sync_fs(c, F, c->tun.mirror_writes && c->tun.copy_kernels);   // n_o per frame (written to the mirror by the scan): picks the clustering path and sizes the launches
    if (st) return st;
    int max_no = 0;
    for (int f = 0; f < F; ++f) max_no = std::max(max_no, c->h_fs[f].n_o);
    int omap_pitch = 0, pmap_pitch = 0;
    // rule C20 (cd_set_table_prism), then rule C16 (cd_set_outlier_filter) - PCL's tabletop order: d_obj and n_o become the kept, then
    // the filtered clouds; max_no stays an upper bound
    if (c->prism_on) st = stage_prism(c, F, max_no, &pmap_pitch);
    if (!st && c->outlier_k > 0) st = stage_outlier(c, F, max_no, &omap_pitch);
    if (!st && c->prism_on && c->outlier_k > 0) st = prism_compose_map(c, F, pmap_pitch);   // (both maps have rows of one pitch: the same max_no)
    if (st) return st;
    st = stage_cluster_sync(c, F, p, max_no);   // sync #4: n_plane, n_o, n_k, ksize, koff (and, filtered, the outlier records; with the prism, its records)
    if (!st && p->icp_use_guess == CD_GUESS_SURFACE) st = surface_guesses(c, F, p, &fr.surface_flag);
    if (st) return st;
    // [3] ICP of every cluster, against one template or all of them
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    front.release();
    BatchClusters cl;
    st = batch_clusters(c, F, &cl);
    if (st) return st;
    BatchIcp bi;
    begin_batch_icp(c, p, F, cl, &bi);
    // rule C24 (cd_set_box_fit): right after the cluster hand-over, on the clusters as clustered.  Its records come back behind the
    // ICP, whose stages end synchronised - or here, one read before the ICP's planning, when the selection decides slots from them
    std::vector<int> sel;
    if (c->box_on) {
        if (cl.rounds_k > 1) {   // (round 0 was extracted by stage_cluster; the ICP drivers extract the later rounds again, as ever)
            st = upload_koffx(c, F, cl, 1);
            if (!st) st = extract_sources(c, p, F, cl, false);
        }
        if (!st) st = stage_box_fit(c, F, cl.first, cl.size, bi.orig_off);
        if (!st && c->box_select_on && p->template_slot < 0 && bi.slots.size() > 1) {
            st = stage_box_fit_collect(c, cl.ncl);
            bool any = false;
            for (int k = 0; !st && k < cl.ncl; ++k) {
                const cd_box_fit& r = c->box_rec[(size_t)k];
                const bool hit = r.status == CD_OK && r.match_slot >= 0;
                sel.push_back(hit ? r.match_slot : -1);
                any = any || hit;
            }
            if (!any) sel.clear();   // (no cluster matched: the all-pairs call, launch for launch)
        }
        if (st) return st;
    }
    if (!sel.empty()) st = icp_selected(c, p, F, cl, &bi, sel);
    else if (fits_one_stage(c, F, cl, (int)bi.slots.size())) st = icp_all_pairs(c, p, F, cl, &bi);
    else st = icp_per_template(c, p, F, cl, &bi);
    if (!st && c->box_on) st = stage_box_fit_collect(c, cl.ncl);   // (a second collect of the same fit finds nothing pending)
    if (!st && c->pair_on) st = stage_pair_scores(c, cl.ncl, bi.orig_off);   // rule C21: after the slot of every cluster is settled
    if (!st && c->pose_on) st = stage_pose_info(c, cl.ncl, bi.orig_off);     // rule C23: reads (points, T, slot) of the same results
    if (st) return st;
    publish_last(c, p, F, cl, &bi);
    {   // what the label calls (rule C15, labels.hip) need of this call; host fields only
        LastCall& lc = c->last_call;
        lc.stride = stride; lc.N = N; lc.F = F;
        lc.prm = *p;
        lc.rects = c->call_rects;
        lc.depth_is_c7 = !(dj && dj->ccam && dj->ccam->no_texture != CD_NOTEX_KEEP);
        lc.keys = c->voxel_keys;
        lc.filtered = c->outlier_k > 0;
        lc.omap_pitch = omap_pitch;
        if (lc.filtered) {   // cd_get_outlier_stats (the records' mirror has been valid since the cluster stage's synchronisation)
            c->last_outlier.assign(c->h_orec.get(), c->h_orec.get() + F);
            c->last_outlier_ok = true;
        }
        lc.prism = c->prism_on != 0;
        if (lc.prism) {   // cd_get_prism_stats / cd_get_prism_hull (as the outlier records; the hulls stay in d_phull)
            lc.omap_pitch = pmap_pitch;
            c->last_prism.assign(c->h_prec.get(), c->h_prec.get() + F);
            c->last_prism_ok = true;
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    // records and read-out
    write_frame_records(c, N, F, cl, fr, results);
    st = copy_frame_indices(c, N, F, plane_inliers, labels);
    if (!st) st = read_stage_timing(c, bi.pairs);
    if (!st) st = publish_bboxes(c, gate_source, F);
    return st;
}

int cd_process_batch_impl(cd_context* c, const void* frames, size_t stride, int points_per_frame, int n_frames,
                     const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    if (!frames || points_per_frame <= 0 || n_frames <= 0) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    const size_t bytes = (size_t)points_per_frame * n_frames * stride;
    int st = check_bbox_source(c, p, n_frames, false);   // (before the upload)
    if (!st && p) st = check_icp_modes(c, p->template_slot);
    if (st) return st;
    st = ensure_input(c, bytes);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, frames, bytes, hipMemcpyHostToDevice, c->stream));
    return process_batch_impl(c, c->d_in, stride, points_per_frame, n_frames, p, results, plane_inliers, labels);
}

// ccam != nullptr: the mapped call (rule C12)
int cd_process_depth_batch_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames,
                                       const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels, bool on_device,
                                       const cd_color_camera* ccam = nullptr, bool mapped = false) {
    int st = check_params(c, p);
    if (st) return st;
    if (!results) return fail(c, CD_ERR_INVALID_ARG, "results is NULL");
    st = mapped ? check_mapped(c, cam, ccam, depth, color, n_frames) : check_depth(c, cam, depth, color, n_frames);
    if (st) return st;
    st = check_bbox_source(c, p, n_frames, cam->color == CD_COLOR_RGB8);   // (before the uploads)
    if (!st) st = check_icp_modes(c, p->template_slot);
    if (st) return st;
    cd_params q = *p;
    q.rgb_offset = cam->color == CD_COLOR_RGB8 ? 12 : -1;   // the canonical records: x y z rgb, 16 bytes
    const int P = cam->width * cam->height;
    st = ensure_input(c, (size_t)P * n_frames * sizeof(float4));
    if (st) return st;
    DepthJob dj{cam, depth, cam->color == CD_COLOR_RGB8 ? color : nullptr, ccam};
    if (!on_device) {
        st = upload_depth(c, cam, depth, color, n_frames, &dj, ccam);
        if (st) return st;
    }
    return process_batch_impl(c, c->d_in, sizeof(float4), P, n_frames, &q, results, plane_inliers, labels, &dj);
}
}  // namespace

extern "C" {
int cd_process_frame(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, cd_frame_result* result,
                     int32_t* plane_inliers, int32_t* labels) {
    return cd_process_batch(c, points, stride, n, 1, p, result, plane_inliers, labels);
}

int cd_get_cluster_results(const cd_context* c, int frame, int first, int capacity, cd_cluster_result* out, int* out_total) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (out_total) *out_total = 0;
    if (frame < 0 || first < 0 || capacity < 0 || (capacity > 0 && !out)) return CD_ERR_INVALID_ARG;
    if ((size_t)frame + 1 >= c->last_first.size()) return CD_ERR_INVALID_ARG;   // not a frame of the last batch
    const int lo = c->last_first[(size_t)frame], hi = c->last_first[(size_t)frame + 1];
    if (lo < 0 || hi < lo || (size_t)hi > c->last_clusters.size()) return CD_ERR_INVALID_ARG;
    if (out_total) *out_total = hi - lo;
    int n = 0;
    for (int k = lo + first; k < hi && n < capacity; ++k) out[n++] = c->last_clusters[(size_t)k];
    return n;
}

int cd_get_frame_cloud(cd_context* c, int frame, int which, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!out_n || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3) || (which != CD_CLOUD_VOXELS && which != CD_CLOUD_OBJECTS) ||
        (rgb_offset >= 0 && (rgb_offset < 12 || (rgb_offset & 3) || (size_t)rgb_offset + 4 > stride)))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (!c->last_clouds || frame < 0 || (size_t)frame >= c->last_nv.size()) return fail(c, CD_ERR_INVALID_ARG, "not a frame of the last fused call of this context");
    const int m = which == CD_CLOUD_VOXELS ? c->last_nv[(size_t)frame] : c->last_no[(size_t)frame];
    if (m > capacity) { *out_n = m; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const float4* src = (which == CD_CLOUD_VOXELS ? c->d_vox : c->d_obj) + (size_t)frame * c->N;
    const int st = download_records(c, src, m, stride, rgb_offset, 0u, out_records);
    if (st) return st;
    *out_n = m;
    return CD_OK;
}

int cd_get_cluster_points(cd_context* c, int frame, int k, int aligned, void* out_points, size_t stride, int capacity, int* out_n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!out_n || capacity < 0 || (capacity > 0 && !out_points) || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (!c->last_clouds || frame < 0 || (size_t)frame + 1 >= c->last_first.size()) return fail(c, CD_ERR_INVALID_ARG, "not a frame of the last fused call of this context");
    const int lo = c->last_first[(size_t)frame], hi = c->last_first[(size_t)frame + 1];
    if (k < 0 || lo + k >= hi || (size_t)(lo + k) >= c->last_clusters.size()) return fail(c, CD_ERR_INVALID_ARG, "no such cluster");
    const cd_cluster_result& r = c->last_clusters[(size_t)(lo + k)];
    const int m = r.size;
    if (m > capacity) { *out_n = m; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const long long o0 = c->last_orig_off[(size_t)(lo + k)], o1 = c->last_al_off[(size_t)(lo + k)];
    const uint32_t one = 0x3f800000u;   // pcl::PointXYZ::data[3]
    int st;
    if (!aligned || o1 >= 0) {
        st = download_records(c, (aligned ? c->d_src : c->d_src0) + (aligned ? o1 : o0), m, stride, -1, one, out_points);
        if (st) return st;
    } else {
        // the pass that produced the best result has been overwritten by a later template pass: final_transformation * cluster
        st = download_records(c, c->d_src0 + o0, m, stride, -1, one, out_points);
        if (st) return st;
        for (int i = 0; i < m; ++i) {
            float v[3];
            char* rec = (char*)out_points + (size_t)i * stride;
            std::memcpy(v, rec, 12);
            const float* T = r.T;
            const float o[3] = {((T[0] * v[0] + T[1] * v[1]) + T[2] * v[2]) + T[3], ((T[4] * v[0] + T[5] * v[1]) + T[6] * v[2]) + T[7],
                                ((T[8] * v[0] + T[9] * v[1]) + T[10] * v[2]) + T[11]};
            std::memcpy(rec, o, 12);
        }
    }
    *out_n = m;
    return CD_OK;
}

int cd_process_batch_device(cd_context* c, const void* d_frames, size_t stride, int points_per_frame, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return process_batch_impl(c, d_frames, stride, points_per_frame, n_frames, p, results, plane_inliers, labels); });
}
int cd_process_batch(cd_context* c, const void* frames, size_t stride, int points_per_frame, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return cd_process_batch_impl(c, frames, stride, points_per_frame, n_frames, p, results, plane_inliers, labels); });
}
int cd_process_depth_batch(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return cd_process_depth_batch_impl(c, cam, depth, color, n_frames, p, results, plane_inliers, labels, false); });
}
int cd_process_depth_batch_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth, const uint8_t* color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return cd_process_depth_batch_impl(c, cam, depth, color, n_frames, p, results, plane_inliers, labels, false, ccam, true); });
}
int cd_process_depth_batch_mapped_device(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* d_depth, const uint8_t* d_color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return cd_process_depth_batch_impl(c, cam, d_depth, d_color, n_frames, p, results, plane_inliers, labels, true, ccam, true); });
}
int cd_process_depth_batch_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, const uint8_t* d_color, int n_frames, const cd_params* p, cd_frame_result* results, int32_t* plane_inliers, int32_t* labels) {
    return with_scan_retry(c, [&] { return cd_process_depth_batch_impl(c, cam, d_depth, d_color, n_frames, p, results, plane_inliers, labels, true); });
}
}  // extern "C"
