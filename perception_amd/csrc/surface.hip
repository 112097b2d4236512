// surface.hip - the batched surface-normal stage (three constrained fits per frame on the S2 / S3 drivers) and the colour stage
#include "context.hpp"
#include "host_math.hpp"

namespace cd {
// ---- batched surface-normal estimation (sne.cpp:167-234 over F frames: cd_surface_batch, CD_GUESS_SURFACE) ----------------
// The three constrained fits run over every frame at once: round i is stage_plane + stage_extract on each frame's current
// cloud, k_surface_centroid sums the plane points, and the leftover cloud (ExtractIndices(negative = invert), what S3 writes to
// its object buffer with extract_negative = invert) is the next round's cloud; a frame whose fit fails drops out.  The stages
// run on the surface stage's own buffers: SurfaceBuffers swaps them in for its lifetime.

int ensure_surface(cd_context* c, size_t pitch) {   // (the per-frame arrays at the context's capacity, the clouds as needed)
    const size_t F = (size_t)c->F, need = F * std::max<size_t>(pitch, 1);
    GROW(c, d_sfs, F); GROW(c, h_sfs, F);
    GROW(c, d_smodel, F); GROW(c, h_smodel, F);
    GROW(c, d_shave, F); GROW(c, h_shave, F);
    GROW(c, d_sactive, F); GROW(c, h_sactive, F);
    GROW(c, d_ssum, 3 * F); GROW(c, h_ssum, 3 * F);
    GROW(c, d_spts[0], need); GROW(c, d_spts[1], need); GROW(c, d_sidx, need);
    return CD_OK;
}

namespace {
// For its lifetime the S2/S3 stage drivers work on the surface stage's buffers: FrameStates, models, have / active flags,
// d_vox = the current clouds (d_spts[0]), d_obj = the next (d_spts[1]), d_plane_idx; row pitch `pitch` points.  Its own
// scratch fills are done by the stages (batch_zeroed off); everything is put back on every way out.
struct SurfaceBuffers {
    cd_context* c;
    int N, T;
    bool zeroed;
    SurfaceBuffers(cd_context* ctx, int pitch) : c(ctx), N(ctx->N), T(ctx->T), zeroed(ctx->batch_zeroed) {
        swap_all();
        c->N = pitch;
        c->T = (pitch + TILE - 1) / TILE;
        c->batch_zeroed = false;
    }
    ~SurfaceBuffers() {
        swap_all();
        c->N = N;
        c->T = T;
        c->batch_zeroed = zeroed;
    }
    void swap_all() {
        std::swap(c->d_fs, c->d_sfs); std::swap(c->h_fs, c->h_sfs);
        std::swap(c->d_model, c->d_smodel); std::swap(c->h_model, c->h_smodel);
        std::swap(c->d_have, c->d_shave); std::swap(c->h_have, c->h_shave);
        std::swap(c->d_active, c->d_sactive); std::swap(c->h_active, c->h_sactive);
        std::swap(c->d_vox, c->d_spts[0]); std::swap(c->d_obj, c->d_spts[1]);
        std::swap(c->d_plane_idx, c->d_sidx);
    }
};
}  // namespace

// in: the clouds in d_spts[0] (rows of `pitch` points), count[f] points each; axes: 3 floats per frame; run[f] = 0: frame f is
// not fitted (status CD_ERR_NO_MODEL, zero record).  q: the fit parameters (threshold, probability) as cd_surface_frame takes them.
int stage_surface(cd_context* c, int F, int pitch, const std::vector<int>& count, const float* axes, const std::vector<char>& run,
                  int invert, const cd_params* p, cd_surface_frame_result* res, int32_t* status) {
    for (int f = 0; f < F; ++f) {
        std::memset(&res[f], 0, sizeof(res[f]));
        status[f] = run[(size_t)f] ? CD_OK : CD_ERR_NO_MODEL;
    }
    const float thr = hm::fold_ge(p->plane_distance_threshold);
    std::vector<int> n(count);
    {
        SurfaceBuffers sb(c, pitch);
        for (int i = 0; i < 3; ++i) {   // sne.cpp:183-197
            cd_params q = *p;
            q.plane_model = i == 0 ? CD_PLANE_PERPENDICULAR : CD_PLANE_PARALLEL;
            q.plane_eps_angle = 0.1;                       // sne.cpp:123
            q.plane_optimize = 1;                          // sne.cpp:118
            q.plane_max_iterations = 1000;                 // sne.cpp:125
            q.extract_negative = invert ? 1 : 0;           // S3's object output = the leftover cloud
            q.crop2_enable = 0;
            q.bbox_enable = 0;
            bool any = false;
            for (int f = 0; f < F; ++f) {   // a fresh FrameState per fit, as load_as gives cd_surface_frame; frames out of the run stay idle
                FrameState& fs = c->h_fs[f];
                std::memset(&fs, 0, sizeof(fs));
                const bool live = status[f] == CD_OK;
                fs.status = live ? CD_OK : CD_ERR_INVALID_ARG;   // (stage_plane fits the frames whose status is OK or NO_MODEL)
                fs.n_v = live ? n[(size_t)f] : 0;
                any = any || live;
            }
            if (!any) break;
            HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState) * F, hipMemcpyHostToDevice));
            std::vector<int> iters;
            int st = stage_plane(c, F, &q, iters, nullptr, axes);
            if (st) return st;
            for (int f = 0; f < F; ++f) {
                if (status[f] != CD_OK) continue;
                res[f].iterations[i] = iters[(size_t)f];
                if (!c->h_have[f]) status[f] = CD_ERR_NO_MODEL;
            }
            st = stage_extract(c, F, &q);
            if (st) return st;
            LAUNCH(c, launch_surface_centroid(c->stream, c->d_vox, pitch, F, c->d_fs, c->tun.mirror_reads ? c->h_model : c->d_model,
                                              c->tun.mirror_reads ? c->h_active : c->d_have, thr, invert, c->d_ssum + i, 3));
            st = sync_fs(c, F, c->tun.mirror_writes && c->tun.copy_kernels);   // n_o: the leftover clouds
            if (st) return st;
            for (int f = 0; f < F; ++f) {
                if (status[f] != CD_OK) continue;
                n[(size_t)f] = c->h_fs[f].n_o;
                const float4 m = c->h_model[f];   // (in fit order; sorted below)
                res[f].coeff[i][0] = m.x; res[f].coeff[i][1] = m.y; res[f].coeff[i][2] = m.z; res[f].coeff[i][3] = m.w;
            }
            std::swap(c->d_vox, c->d_obj);
        }
    }
    HIPCHK(c, xfer(c, c->h_ssum, c->d_ssum, sizeof(float4) * 3 * (size_t)F, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < F; ++f) {
        cd_surface_frame_result& r = res[f];
        if (status[f] != CD_OK) {   // (a failed fit leaves the iterations of the fits run so far and nothing else)
            std::memset(r.coeff, 0, sizeof(r.coeff));
            continue;
        }
        float normals[3][4], mids[3][4];
        int counts[3];
        for (int i = 0; i < 3; ++i) {
            const float4 sm = c->h_ssum[3 * (size_t)f + i];
            std::memcpy(&counts[i], &sm.w, 4);
            const float cnt = (float)counts[i];   // pcl::compute3DCentroid: the sums / the count
            mids[i][0] = sm.x / cnt; mids[i][1] = sm.y / cnt; mids[i][2] = sm.z / cnt; mids[i][3] = 0.f;
            for (int a = 0; a < 4; ++a) normals[i][a] = r.coeff[i][a];
        }
        surface_record(counts, normals, mids, &r);
    }
    return CD_OK;
}

// sne.cpp:199-212: the three fits ordered by size (the callback's own exchange loops), largest first, and the pose from them
void surface_record(int counts[3], float normals[3][4], float mids[3][4], cd_surface_frame_result* r) {
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j)
            if (counts[i] < counts[j]) {
                std::swap(counts[i], counts[j]);
                for (int a = 0; a < 4; ++a) { std::swap(normals[i][a], normals[j][a]); std::swap(mids[i][a], mids[j][a]); }
            }
    hm::surface_frame(normals, mids, r->Rt);
    for (int i = 0; i < 3; ++i) {
        r->n_points[i] = counts[i];
        for (int a = 0; a < 4; ++a) { r->coeff[i][a] = normals[i][a]; r->midpoint[i][a] = mids[i][a]; }
    }
}

// CD_GUESS_SURFACE: the surface fit of every frame that has a ground plane, on its objects cloud (d_obj, n_o), table normal =
// its plane, invert = 1, the context's threshold -> c->last_surface*; rule C9 -> c->surface_guess (identity where the fit
// fails); (*flagged)[f] = 1 where the guess came from the fit
int surface_guesses(cd_context* c, int F, const cd_params* p, std::vector<char>* flagged) {
    std::vector<int> count((size_t)F, 0);
    std::vector<char> run((size_t)F, 0);
    std::vector<float> axes(3 * (size_t)F, 0.f);
    int pitch = 1;
    for (int f = 0; f < F; ++f) {
        if (!c->h_have[f]) continue;
        run[(size_t)f] = 1;
        count[(size_t)f] = c->h_fs[f].n_o;
        pitch = std::max(pitch, count[(size_t)f]);
        axes[3 * (size_t)f] = c->h_model[f].x; axes[3 * (size_t)f + 1] = c->h_model[f].y; axes[3 * (size_t)f + 2] = c->h_model[f].z;
    }
    int st = ensure_surface(c, (size_t)pitch);
    if (st) return st;
    LAUNCH(c, launch_surface_load(c->stream, c->d_obj, sizeof(float4), sizeof(float4) * (size_t)c->N, FS_FIELD(c, n_o), FS_PITCH, pitch, pitch, F, c->d_spts[0]));
    cd_params q = *p;
    q.plane_distance_threshold = c->surface_thr;
    c->last_surface.assign((size_t)F, cd_surface_frame_result());
    c->last_surface_status.assign((size_t)F, CD_ERR_NO_MODEL);
    st = stage_surface(c, F, pitch, count, axes.data(), run, 1, &q, c->last_surface.data(), c->last_surface_status.data());
    if (st) return st;
    c->surface_guess.assign(16 * (size_t)F, 0.f);
    flagged->assign((size_t)F, 0);
    for (int f = 0; f < F; ++f) {
        float* g = c->surface_guess.data() + 16 * (size_t)f;
        for (int i = 0; i < 4; ++i) g[5 * i] = 1.f;
        float h[16];
        if (c->last_surface_status[(size_t)f] == CD_OK && cd_surface_guess(c->last_surface[(size_t)f].Rt, h) == CD_OK) {
            std::memcpy(g, h, sizeof(h));
            (*flagged)[(size_t)f] = 1;
        }
    }
    return CD_OK;
}

// ---- colour gate (rule C10, k_color.hip) ---------------------------------------------------------------------------------------
static_assert(sizeof(ColorRecord) == sizeof(cd_color_bbox) && offsetof(ColorRecord, rect) == 0 && offsetof(cd_color_bbox, rect) == 0, "the kernel's record is cd_color_bbox");
int check_color_params(cd_context* c, const cd_color_gate_params* g) {
    if (g->h_lo_max < 0 || g->h_lo_max > 179 || g->h_hi_min < 0 || g->h_hi_min > 179) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the H bounds must be in 0 .. 179");
    if (g->s_min < 0 || g->s_min > 255 || g->v_min < 0 || g->v_min > 255) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the S and V minima must be in 0 .. 255");
    if (g->margin < 0) return fail(c, CD_ERR_INVALID_ARG, "colour gate: the margin must not be negative");
    return CD_OK;
}

// the rectangles of F rgb8 images (device-resident, W x H each) into d_crec / d_cstatus, and on into their pinned mirrors
// (valid after the next synchronisation of the context's stream)
int stage_color(cd_context* c, const uint8_t* d_rgb, int W, int H, int F, const cd_color_gate_params* g) {
    const size_t px = (size_t)W * H;
    if (c->d_clabel.capacity() < px * F) GROW(c, d_clabel, std::max(px * F, std::min((size_t)c->N * c->F, (size_t)640 * 480 * c->F)));
    uint32_t* gmask = nullptr;
    if (!color_fits_lds(W, H)) {
        GROW(c, d_cmask, 2 * (size_t)((W + 31) / 32) * H * F);
        gmask = c->d_cmask;
    }
    const ColorGate cg{g->h_lo_max, g->h_hi_min, g->s_min, g->v_min, g->margin};
    LAUNCH(c, launch_color_bbox(c->stream, d_rgb, W, H, F, cg, c->d_ctab, gmask, c->d_clabel, px, c->d_crec, c->d_cstatus));
    HIPCHK(c, xfer(c, c->h_crec, c->d_crec, sizeof(ColorRecord) * (size_t)F, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_cstatus, c->d_cstatus, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost));
    return CD_OK;
}

// after the synchronisation: a border walk that ran out of steps (cannot happen: the bound is every (pixel, direction) pair)
int color_status(cd_context* c, int F) {
    for (int f = 0; f < F; ++f)
        if (c->h_cstatus[f] != CD_OK) return fail(c, CD_ERR_CAPACITY, "colour gate: a border walk exceeded its step bound");
    return CD_OK;
}
}  // namespace cd
