// cuboid_hip.hip - the stage drivers of the pipeline, device-resident in and out: S0 .. S5 (crop + voxel grid, plane, extract,
// cluster) and S6 (the ICP planner and its five drivers).  The fused call (batch.hip) and the entries (entries.hip) run them.
#include "context.hpp"
#include "host_math.hpp"

namespace cd {

// ---- stage drivers (device-resident in/out; F frames) ------------------------------------

// S0+S1.  in: F*N records of `stride` bytes on the device.  out: d_vox / fs.n_v
int stage_crop_voxel(cd_context* c, const void* d_in, size_t stride, int N, int F, const cd_params* p, int* rounds_out) {
    const int T = c->T;
    CropLimits lim;
    lim.zlo = hm::fold_ge(p->crop_z_min);
    lim.zhi = hm::fold_le(p->crop_z_max);
    lim.xlo = hm::fold_ge(p->crop_x_min);
    lim.xhi = hm::fold_le(p->crop_x_max);
    const int rgb_off = (p->rgb_offset >= 0 && (size_t)p->rgb_offset + 4 <= stride) ? p->rgb_offset : -1;
    // FrameState init: status 0, mn = +max, mx = 0 (ordered-uint encoding)
    auto init_fs = [&] {
        for (int f = 0; f < F; ++f) {
            FrameState& s = c->h_fs[f];
            std::memset(&s, 0, sizeof(s));
            for (int a = 0; a < 3; ++a) { s.mn[a] = 0xffffffffu; s.mx[a] = 0u; }
        }
    };
    init_fs();
    // Single pass (one read of the input) when the crop limits bound the x and z cell indices tightly enough to leave the
    // unbounded y index a wide bit field; a frame whose y does not fit anyway sends the batch through the two-pass path.
    KeyPack kp;
    std::memset(&kp, 0, sizeof(kp));
    {
        const float inv = 1.0f / p->leaf_size;
        const float fl[4] = {std::floor(lim.xlo * inv), std::floor(lim.xhi * inv), std::floor(lim.zlo * inv), std::floor(lim.zhi * inv)};
        bool ok = !c->tun.crop_two_pass;
        for (float v : fl) ok = ok && std::fabs(v) < 1.0e9f;
        if (ok && fl[1] >= fl[0] && fl[3] >= fl[2]) {
            const long long ri = (long long)fl[1] - (long long)fl[0] + 1, rk = (long long)fl[3] - (long long)fl[2] + 1;
            int bi = 1, bk = 1;
            while ((1ll << bi) < ri) ++bi;
            while ((1ll << bk) < rk) ++bk;
            if (bi + bk <= 20) {
                kp.enabled = 1;
                kp.bi = bi; kp.bj = 32 - bi - bk;
                kp.ilo = (int)fl[0]; kp.klo = (int)fl[2]; kp.jlo = -(1 << (kp.bj - 1));
                // y = 0 sits 256 cells above an aligned block of 512 field values: a frame whose y cells stay within +-256 of the
                // optical axis (1.28 m at the 5 mm leaf) then has constant y bits above the ninth, and the sort of k_crop_runs,
                // which runs on these packed keys, skips the digit they fill (3 passes instead of 4 on the bench frames; with y = 0
                // ON a block boundary every frame straddles it)
                if (kp.bj >= 11) kp.jlo -= 256;
            }
        }
    }
    // Round 4: the single-pass crop also writes the RUNS (one record per run of equal cell key inside a row of 64 input points)
    // and their digit histograms, and the sort runs on the packed cell keys themselves (k_crop_runs, k_voxel.hip)
    bool crop_runs = kp.enabled && c->tun.crop_runs && c->tun.voxel_runs && c->N <= (1 << RUN_SHIFT);
    // 16-byte records x y z rgb (the D435 driver's layout): k_crop_runs leaves the kept points where they are and the centroid
    // kernel reads the input (0.5 GB less written and the same bytes read per 256-frame batch); any other layout is copied
    const bool direct_pts = c->tun.crop_direct && stride == 16 && (rgb_off == 12 || rgb_off < 0) && (reinterpret_cast<uintptr_t>(d_in) & 15u) == 0;
    int st = CD_OK;
    // (the ticket counters reset themselves at the end of every launch that uses them; zeroed here too so that a call that
    // failed half way can never leave the next one with a counter that is not zero)
    ZERO_FILL(c, c->d_ticket, sizeof(int) * (size_t)F * TICKET_PITCH);
    // (kernels write the pinned mirror of the FrameState array themselves where a whole copy launch used to follow them:
    // CUBOID_MIRROR_WRITES=0 restores the copies)
    FrameState* const fs_mirror = c->tun.mirror_writes && c->tun.copy_kernels ? c->h_fs : nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!(attempt == 0 && c->fs_initialised)) HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState) * F, hipMemcpyHostToDevice));   // (a fused call's zero launch set them)
        c->fs_initialised = false;
        // (the rare redo, and the crops that use d_tileA themselves: from here on every stage fills its own arrays again)
        if (attempt > 0 || !(kp.enabled && crop_runs)) c->batch_zeroed = false;
        ZERO_FILL(c, c->d_tileA, sizeof(int) * (size_t)F * T);
        if (kp.enabled && crop_runs) {
            ZERO_FILL(c, c->d_tile64, sizeof(unsigned long long) * (size_t)F * T);
            ZERO_FILL(c, c->d_ghist, sizeof(uint32_t) * (size_t)F * SORT_MAX_PASSES_HOST * RADIX);
            LAUNCH(c, launch_crop_runs(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, kp, c->d_fs, c->d_tile64, c->d_cpt, c->d_key[0], c->d_val[0],
                             c->d_ghist, c->d_ticket, direct_pts ? 1 : 0));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, c->d_ghist, fs_mirror));
        } else if (kp.enabled) {
            LAUNCH(c, launch_crop_fused(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, kp, c->d_fs, c->d_tileA, c->d_cpt, c->d_key[0], c->d_ticket));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, nullptr, fs_mirror));
        } else {
            LAUNCH(c, launch_crop_count(c->stream, d_in, stride, N, F, rgb_off, lim, T, c->d_fs, c->d_tileA));
            LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileA, F, T, FS_FIELD(c, n_c), FS_PITCH));
            LAUNCH(c, launch_voxel_setup(c->stream, c->d_fs, F, p->leaf_size, nullptr, fs_mirror));
            LAUNCH(c, launch_crop_compact(c->stream, d_in, stride, N, c->N, F, rgb_off, lim, T, p->leaf_size, c->d_fs, c->d_tileA, c->d_cpt, c->d_key[0]));
        }
        st = sync_fs(c, F, fs_mirror != nullptr);   // sync #1: n_c, key_bits (sort pass count); the mirror was written by k_voxel_setup
        if (st) return st;
        bool over = false;
        for (int f = 0; f < F; ++f) over = over || c->h_fs[f].crop_overflow != 0;
        if (!over) break;
        if (std::getenv("CUBOID_DEBUG")) std::fprintf(stderr, "cuboid_hip: single-pass crop overflowed, redoing the batch in two passes\n");
        kp.enabled = 0;       // rare: redo the crop in two passes (the FrameState init in h_fs was overwritten by the sync)
        crop_runs = false;
        init_fs();
    }
    int max_nc = 0, max_bits = 0;
    for (int f = 0; f < F; ++f) { max_nc = std::max(max_nc, c->h_fs[f].n_c); max_bits = std::max(max_bits, c->h_fs[f].key_bits); }
    const int Tc = std::max(1, (max_nc + TILE - 1) / TILE);
    const int Tsc = std::max(1, (max_nc + SORT_TILE - 1) / SORT_TILE);          // tiles of k_voxel_runs / k_radix_ghist
    const int Tscat = std::max(1, (max_nc + SCATTER_TILE - 1) / SCATTER_TILE);   // tiles of the scatters (their own size: common.hpp)
    const int npass = (max_bits + RADIX_BITS - 1) / RADIX_BITS;
    int cur = 0;
    // By runs (default): the sort moves one element per run of equal voxel index among the cropped points - they are in image
    // order, 2.4 points per run on the bench frames - and the centroid kernel reads the runs' points contiguously; the bound
    // on the tiles is the point count (the run count is only known on the device).  CUBOID_VOXEL_RUNS=0: sort the points.
    const bool by_runs = c->tun.voxel_runs && npass > 0 && c->N <= (1 << RUN_SHIFT);   // (a run's start takes RUN_SHIFT bits of its payload)
    int Tc_runs = Tc;
    uint32_t* const key[2] = {c->d_key[0], c->d_key[1]}, * const val[2] = {c->d_val[0], c->d_val[1]};
    if (crop_runs) {
        // the runs and their histograms are there already; which of the packed key's four digits vary in some frame?
        int vary = 0, max_runs = 0;
        for (int f = 0; f < F; ++f) {
            if (c->h_fs[f].n_c > 0) vary |= c->h_fs[f].digit_vary;
            max_runs = std::max(max_runs, c->h_fs[f].n_runs);
        }
        int digits[4], nd = 0;
        for (int d = 0; d < 4; ++d) if ((vary >> d) & 1) digits[nd++] = d;
        const int Tsr = std::max(1, (max_runs + SCATTER_TILE - 1) / SCATTER_TILE);   // (the run count is known here: tighter than the point count)
        Tc_runs = std::max(1, (max_runs + TILE - 1) / TILE);
        LAUNCH(c, cur = launch_radix_scatter_runs(c->stream, key, val, c->N, F, Tsr, digits, nd, c->d_fs, c->d_ghist, c->d_sstate, c->d_ticket));
    } else if (by_runs)
        LAUNCH(c, cur = launch_radix_sort_runs(c->stream, key, val, c->N, F, T, Tsc, Tscat, npass, c->d_fs, c->d_ghist, c->d_sstate, c->d_tileA, kp, c->d_ticket));
    else
        LAUNCH(c, cur = launch_radix_sort(c->stream, key, val, c->N, F, Tsc, Tscat, npass, c->d_fs, c->d_ghist, c->d_sstate, kp, c->d_ticket));
    if (cur < 0) return fail(c, CD_ERR_DEVICE, "radix sort: the scan state could not be zeroed");
    const uint32_t* vin = c->d_val[cur];   // zero passes (empty frames only): the permutation is never read
    // voxel heads + centroids in one kernel: n_v (0 from the FrameState init for empty frames) and every tile's output
    // offset come from a chained scan (state in d_tileA)
    ZERO_FILL(c, c->d_tileC, sizeof(int) * (size_t)F * T);
    if (crop_runs || by_runs)
        LAUNCH(c, launch_voxel_centroid_runs(c->stream, c->d_key[cur], vin, crop_runs && direct_pts ? reinterpret_cast<const float4*>(d_in) : c->d_cpt, c->N, F, T, crop_runs ? Tc_runs : Tc,
                                             rgb_off >= 0 ? 1 : 0, c->d_fs, c->d_tileC, c->d_vox, c->d_ticket, c->tun.centroid_lanes, crop_runs && direct_pts ? N : c->N));
    else
        LAUNCH(c, launch_voxel_centroid(c->stream, c->d_key[cur], vin, c->d_cpt, c->N, F, T, Tc, rgb_off >= 0 ? 1 : 0, c->d_fs, c->d_tileC, c->d_vox, c->d_ticket));
    // (rule C15: where the sorted keys are and what they are)
    c->voxel_keys.cur = cur;
    c->voxel_keys.by_runs = (crop_runs || by_runs) ? 1 : 0;
    c->voxel_keys.packed = crop_runs ? 1 : 0;
    c->voxel_keys.kp = kp;
    c->voxel_keys.path = crop_runs ? (direct_pts ? "runs direct" : "runs compacted") : (by_runs ? (kp.enabled ? "fused single pass" : "two-pass") : "sort by points");
    if (rounds_out) *rounds_out = 0;
    return CD_OK;
}

// S2.  in: d_vox + fs.n_v (host mirror h_fs[].n_v must be current).  out: h_model/h_have refined,
// fs.status updated for NO_MODEL, iterations per frame.
// axes: per-frame constraint axes of a constrained model, 3 floats per frame (nullptr: p->plane_axis for every frame)
int stage_plane(cd_context* c, int F, const cd_params* p, std::vector<int>& iterations, int* rounds_out, const float* axes) {
    const int T = c->T;
    const bool mr = c->tun.mirror_reads != 0;
    const float thr = hm::fold_ge(p->plane_distance_threshold);
    int max_nv = 0;
    for (int f = 0; f < F; ++f) max_nv = std::max(max_nv, c->h_fs[f].n_v);
    const int Tv = std::max(1, (max_nv + TILE - 1) / TILE);
    std::vector<hm::RansacReplay> rep(F);
    iterations.assign(F, 0);
    for (int f = 0; f < F; ++f) c->h_active[f] = (c->h_fs[f].status == CD_OK || c->h_fs[f].status == CD_ERR_NO_MODEL) ? 1 : 0;
    ZERO_FILL(c, c->d_counts, sizeof(int) * (size_t)F * MAX_HYP);
    const int targets[4] = {16, 64, 256, MAX_HYP};
    const int h_cap = std::min(MAX_HYP, p->plane_max_iterations + 40);   // max_iterations+1 plus 39 skipped models
    int h_prev = 0, rounds = 0;
    for (int r = 0; r < 4; ++r) {
        const int h_target = std::min(targets[r], h_cap);
        if (h_target <= h_prev) break;
        // (mirror reads: the kernels read the few per-frame words the host decides - active flags, chosen models - straight from
        // the pinned host arrays, which the device sees; CUBOID_MIRROR_READS=0 uploads them first as rounds 1-5 did)
        if (!mr) HIPCHK(c, xfer(c, c->d_active, c->h_active, sizeof(int) * F, hipMemcpyHostToDevice));
        const int* active_p = mr ? c->h_active : c->d_active;
        // (the rounds of 16 and 64 hypotheses with the sampler's 8 KiB map; should a frame's map fill up it moves to the frame's
        // part of the spill area: context.hpp)
        LAUNCH(c, launch_ransac_sample(c->stream, c->d_vox, c->N, F, c->d_fs, c->d_rnd, h_target, active_p, c->d_models, c->d_valid,
                                       c->tun.cluster_tiers ? sampler_spill_area(c) : nullptr, SAMPLER_SPILL_PITCH));
        LAUNCH(c, launch_ransac_count(c->stream, c->d_vox, c->N, F, Tv, c->d_fs, c->d_models, c->d_valid, active_p, h_prev, h_target, thr, c->d_counts));
        // only the first h_target columns of the [F][MAX_HYP] tables are live: one strided copy each
        {   // (one launch: the three tables and - sync_fs below finds it done - nothing else; the FrameState read-back follows)
            XferBatch xb(c);
            xb.add2d(c->h_counts, sizeof(int) * MAX_HYP, c->d_counts, sizeof(int) * MAX_HYP, sizeof(int) * h_target, F, hipMemcpyDeviceToHost);
            xb.add2d(c->h_valid, sizeof(int) * MAX_HYP, c->d_valid, sizeof(int) * MAX_HYP, sizeof(int) * h_target, F, hipMemcpyDeviceToHost);
            xb.add2d(c->h_models, sizeof(float4) * MAX_HYP, c->d_models, sizeof(float4) * MAX_HYP, sizeof(float4) * h_target, F, hipMemcpyDeviceToHost);
            xb.add(c->h_fs, c->d_fs, sizeof(FrameState) * F, hipMemcpyDeviceToHost);
            HIPCHK(c, xb.flush());
        }
        int st = sync_fs(c, F, /*copied=*/true);   // sync #2 (per round): counts + n_hyp
        if (st) return st;
        ++rounds;
        bool all_done = true;
        for (int f = 0; f < F; ++f) {
            if (!c->h_active[f]) continue;
            const FrameState& s = c->h_fs[f];
            if (p->plane_model != CD_PLANE) {   // constrained models: a hypothesis off the axis constraint scores 0 inliers
                for (int h = rep[f].pos; h < s.n_hyp; ++h) {
                    const float4 m = c->h_models[(size_t)f * MAX_HYP + h];
                    const float mm[4] = {m.x, m.y, m.z, m.w};
                    if (c->h_valid[(size_t)f * MAX_HYP + h] && !hm::plane_model_valid(p->plane_model, mm, axes ? axes + 3 * f : p->plane_axis, p->plane_eps_angle))
                        c->h_counts[(size_t)f * MAX_HYP + h] = 0;
                }
            }
            const bool fin = rep[f].consume(c->h_counts + (size_t)f * MAX_HYP, c->h_valid + (size_t)f * MAX_HYP, s.n_hyp, std::max(1, s.n_v),
                                            p->plane_max_iterations, p->plane_probability, s.sampler_exhausted != 0 || h_target >= h_cap);
            if (fin) c->h_active[f] = 0; else all_done = false;
        }
        h_prev = h_target;
        if (all_done) break;
    }
    if (rounds_out) *rounds_out = rounds;
    // chosen models -> device; moments of their inliers -> host eigen33 -> refined models
    for (int f = 0; f < F; ++f) {
        iterations[f] = rep[f].iterations;
        c->h_have[f] = rep[f].best_h >= 0 ? 1 : 0;
        c->h_model[f] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c->h_have[f]) c->h_model[f] = c->h_models[(size_t)f * MAX_HYP + rep[f].best_h];
    }
    // selectWithinDistance of a constrained model returns nothing when the model violates the constraint: the
    // device then sees "no model" (h_active doubles as the pinned staging copy), the host keeps reporting it
    auto upload_have = [&](const float4* models_too = nullptr) -> int {
        for (int f = 0; f < F; ++f) {
            const float mm[4] = {c->h_model[f].x, c->h_model[f].y, c->h_model[f].z, c->h_model[f].w};
            c->h_active[f] = c->h_have[f] && hm::plane_model_valid(p->plane_model, mm, axes ? axes + 3 * f : p->plane_axis, p->plane_eps_angle) ? 1 : 0;
        }
        if (mr) return CD_OK;   // (the kernels read h_model / h_active)
        XferBatch xb(c);
        if (models_too) xb.add(c->d_model, models_too, sizeof(float4) * F, hipMemcpyHostToDevice);
        xb.add(c->d_have, c->h_active, sizeof(int) * F, hipMemcpyHostToDevice);
        HIPCHK(c, xb.flush());
        return CD_OK;
    };
    if (int st = upload_have(&c->h_model[0])) return st;   // (the chosen models ride along: one launch)
    if (p->plane_optimize) {
        ZERO_FILL(c, c->d_sums, sizeof(unsigned long long) * 10 * F);
        LAUNCH(c, launch_plane_cov(c->stream, c->d_vox, c->N, F, Tv, c->d_fs, mr ? c->h_model : c->d_model, mr ? c->h_active : c->d_have, thr, c->d_sums));
        HIPCHK(c, xfer(c, c->h_sums, c->d_sums, sizeof(unsigned long long) * 10 * F, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // sync #3
        for (int f = 0; f < F; ++f) {
            if (!c->h_have[f]) continue;
            float in[4] = {c->h_model[f].x, c->h_model[f].y, c->h_model[f].z, c->h_model[f].w}, out[4];
            hm::plane_refit_from_moments((const uint64_t*)(c->h_sums + 10 * (size_t)f), in, out);
            c->h_model[f] = make_float4(out[0], out[1], out[2], out[3]);
        }
        if (!mr) HIPCHK(c, xfer(c, c->d_model, c->h_model, sizeof(float4) * F, hipMemcpyHostToDevice));
        if (p->plane_model != CD_PLANE) {
            HIPCHK(c, hipStreamSynchronize(c->stream));   // h_active is about to be rewritten
            if (int st = upload_have()) return st;
        }
    }
    (void)T;
    return CD_OK;
}

ExtractArgs extract_args(const cd_params* p, int gate_mode) {
    ExtractArgs ea;
    ea.thr = hm::fold_ge(p->plane_distance_threshold);
    ea.z2lo = hm::fold_ge(p->crop2_z_min);
    ea.z2hi = hm::fold_le(p->crop2_z_max);
    std::memset(&ea.gate, 0, sizeof(ea.gate));
    ea.gate.enable = gate_mode >= 0 ? gate_mode : (p->bbox_enable ? 1 : 0);
    for (int i = 0; i < 12; ++i) ea.gate.P[i] = p->bbox_P[i];
    for (int i = 0; i < 4; ++i) ea.gate.rect[i] = (float)p->bbox_rect[i];
    return ea;
}

// S3 (+S3b).  out: d_plane_idx, d_obj, fs.n_plane, fs.n_o
int stage_extract(cd_context* c, int F, const cd_params* p, int gate_mode) {
    const int T = c->T;
    int max_nv = 0;
    for (int f = 0; f < F; ++f) max_nv = std::max(max_nv, c->h_fs[f].n_v);
    const int Tv = std::max(1, (max_nv + TILE - 1) / TILE);
    const ExtractArgs ea = extract_args(p, gate_mode);
    const float thr = ea.thr, z2lo = ea.z2lo, z2hi = ea.z2hi;
    const BBoxGate& gate = ea.gate;
    const float4* model_p = c->tun.mirror_reads ? c->h_model : c->d_model;   // (see stage_plane)
    const int* have_p = c->tun.mirror_reads ? c->h_active : c->d_have;
    ZERO_FILL(c, c->d_tileA, sizeof(int) * (size_t)F * T);
    ZERO_FILL(c, c->d_tileB, sizeof(int) * (size_t)F * T);
    LAUNCH(c, launch_plane_flag_count(c->stream, c->d_vox, c->N, F, T, Tv, c->d_fs, model_p, have_p, thr, p->extract_negative, p->crop2_enable, z2lo, z2hi, gate, c->call_rects, c->d_tileA, c->d_tileB));
    {   // both scans in one launch; the two totals also go straight into the host's FrameState mirror (nothing else of it changes here)
        const bool mirrored = c->tun.mirror_writes && c->tun.copy_kernels;
        const ScanJob ja{c->d_tileA, FS_FIELD(c, n_plane), mirrored ? (int*)((char*)c->h_fs.get() + offsetof(FrameState, n_plane)) : nullptr};
        const ScanJob jb{c->d_tileB, FS_FIELD(c, n_o), mirrored ? (int*)((char*)c->h_fs.get() + offsetof(FrameState, n_o)) : nullptr};
        LAUNCH(c, launch_scan_tiles2(c->stream, ja, jb, F, T, FS_PITCH));
    }
    LAUNCH(c, launch_extract_scatter(c->stream, c->d_vox, c->N, F, T, Tv, c->d_fs, model_p, have_p, thr, p->extract_negative, p->crop2_enable, z2lo, z2hi, gate, c->call_rects, c->d_tileA, c->d_tileB, c->d_plane_idx, c->d_obj));
    return CD_OK;
}

// S5.  in: d_obj + fs.n_o (device).  out: d_label, d_sizes, fs.n_k/ksize/koff, d_src0/d_src
// level: which kernels cluster the frames.  CL_LEVEL_TIER: the small tier alone (every frame has at most CL_TIER_CAP points);
// CL_LEVEL_TOP: k_cluster_lds, and k_cluster_cells behind it when a frame has more than 8192 points; CL_LEVEL_GLOBAL: the same
// with the point-graph kernels behind them.  A frame that a level gives up (fs.cl_done == 0) is taken by the next one.
enum { CL_LEVEL_TIER = 0, CL_LEVEL_TOP = 1, CL_LEVEL_GLOBAL = 2 };
static int stage_cluster(cd_context* c, int F, const cd_params* p, int max_no_hint, int level) {
    const int T = c->T;
    const int To = std::max(1, (max_no_hint + TILE - 1) / TILE);
    const float cell = (float)(p->cluster_tolerance * (1.0 + 1.0 / 1024.0));
    const float inv_cell = 1.0f / cell;
    const float r2 = (float)(p->cluster_tolerance * p->cluster_tolerance);
    const float small_cell = (float)(p->cluster_tolerance / std::sqrt(3.0) * (1.0 - 1.0 / 1024.0));
    const bool force_global = level == CL_LEVEL_GLOBAL;
    if (p->cluster_enable && level == CL_LEVEL_TIER) {
        // the same cell graph as below with the cell table in 27 KiB of LDS and the points in cell order in d_src (free until the
        // labels are scattered; 70 KB per frame: it stays in L2): a workgroup that finds room beside the other batches' kernels
        LAUNCH(c, launch_cluster_tier(c->stream, c->d_obj, c->N, F, c->d_fs, 1.0f / small_cell, r2, c->d_parent, c->d_csize, c->d_rank, c->d_src));
    } else if (p->cluster_enable) {
        // frames with <= 8192 object points (the usual case) are clustered by one workgroup in LDS, over cells small
        // enough (edge just under tol / sqrt(3)) that the points of one cell are connected by construction ...
        LAUNCH(c, launch_cluster_lds(c->stream, c->d_obj, c->N, F, c->d_fs, 1.0f / small_cell, r2, c->d_parent, c->d_csize, c->d_rank));
    }
    const bool by_cells = c->tun.cluster_cells && !force_global;
    if (p->cluster_enable && max_no_hint > 8192 && by_cells) {
        // ... larger ones by the same cell graph with the points in global memory (k_cluster_cells; d_src is free until the labels
        // are scattered) ...
        LAUNCH(c, launch_cluster_cells(c->stream, c->d_obj, c->N, F, c->d_fs, 1.0f / small_cell, r2, c->d_parent, c->d_csize, c->d_rank, c->d_src));
    }
    if (p->cluster_enable && ((max_no_hint > 8192 && !by_cells) || force_global)) {
        // ... and the rare frame whose cells do not fit the table (fs.cl_done == 0) by the point-graph kernels in global memory
        HIPCHK(c, hipMemsetAsync(c->d_head, 0xff, sizeof(int) * (size_t)F * CELL_BUCKETS, c->stream));
        LAUNCH(c, launch_cluster_build(c->stream, c->d_obj, c->N, F, To, c->d_fs, inv_cell, c->d_head, c->d_next, c->d_parent, c->d_csize, c->d_rank));
        LAUNCH(c, launch_cluster_hook(c->stream, c->d_obj, c->N, F, To, c->d_fs, inv_cell, r2, c->d_head, c->d_next, c->d_parent));
        LAUNCH(c, launch_cluster_flatten(c->stream, c->N, F, To, c->d_fs, c->d_parent, c->d_csize));
    }
    LAUNCH(c, launch_cluster_rank(c->stream, c->N, F, c->d_fs, p->cluster_enable, p->cluster_min_size, p->cluster_max_size, c->d_parent, c->d_csize, c->d_cand, c->d_rank, c->d_sizes, c->tun.mirror_writes && c->tun.copy_kernels ? c->h_fs : nullptr));
    ZERO_FILL(c, c->d_tileK, sizeof(int) * (size_t)F * KICP * T);
    LAUNCH(c, launch_label_count(c->stream, c->N, F, T, To, c->d_fs, p->cluster_enable, c->d_parent, c->d_rank, c->d_label, c->d_tileK, 0));
    LAUNCH(c, launch_scan_tiles(c->stream, c->d_tileK, F * KICP, T, nullptr, 0));
    LAUNCH(c, launch_label_scatter(c->stream, c->d_obj, c->N, F, T, To, c->d_fs, c->d_label, c->d_tileK, c->d_src0, c->d_src, 0, nullptr));
    return CD_OK;
}

// stage_cluster + sync; when the LDS kernel gave a frame up (too many cells / too wide a cloud for its table) and the
// global-memory kernels were not part of the launch, the stage is run again with them.  The first launch is the small tier's
// when the largest frame fits it (CUBOID_CLUSTER_TIERS=0: never); what that gives up goes to k_cluster_lds first.
int stage_cluster_sync(cd_context* c, int F, const cd_params* p, int max_no) {
    const bool mirrored = c->tun.mirror_writes && c->tun.copy_kernels;   // (k_cluster_rank wrote the FrameState mirror)
    int level = c->tun.cluster_tiers && max_no <= CL_TIER_CAP ? CL_LEVEL_TIER : CL_LEVEL_TOP;
    for (;;) {
        int st = stage_cluster(c, F, p, max_no, level);
        if (st) return st;
        st = sync_fs(c, F, mirrored);
        if (st || !p->cluster_enable || level == CL_LEVEL_GLOBAL) return st;
        if (level == CL_LEVEL_TOP && max_no > CL_TOP_CAP && !c->tun.cluster_cells) return st;   // (the point-graph kernels were part of the launch)
        bool left = false;
        for (int f = 0; f < F; ++f) left = left || (c->h_fs[f].n_o > 0 && !c->h_fs[f].cl_done);
        if (!left) return CD_OK;
        ++level;
        if (std::getenv("CUBOID_DEBUG"))
            std::fprintf(stderr, "cuboid_hip: LDS clustering gave frames up, running %s\n", level == CL_LEVEL_TOP ? "the top tier" : "the global-memory path");
        c->batch_zeroed = false;   // (d_tileK has been used: the redo fills it again)
    }
}

// IcpCluster records h_cl[first .. first + n) of the clusters 0 .. n-1 of one frame against template `slot`: sizes size[0..n),
// sources at base + off[0..n) in d_src0 / d_src
void set_icp_clusters(cd_context* c, int first, int n, int frame, const int* size, const int* off, int base, int slot) {
    for (int k = 0; k < n; ++k) c->h_cl[first + k] = IcpCluster{base + off[k], size[k], frame, k, c->tpl_off[slot], c->tpl_m[slot], 0, slot};
}

// the record of a slot's template as the device table holds it: an empty slot can give no guess
ShapeFrame template_frame(const cd_context* c, int slot) {
    if (slot >= 0 && slot < CD_MAX_TEMPLATES && c->tpl_m[slot] > 0) return c->tpl_frame[slot];
    ShapeFrame none;
    shape_empty(0, CD_ERR_NO_TEMPLATE, &none);
    return none;
}

// ---- S6: ICP ------------------------------------------------------------------------------------------------------------------
// stage_icp plans the stage on the host (plan_icp), issues what every driver needs (icp_setup), then hands the clusters to the
// drivers in turn: k_icp_lat for lattice templates, the grouped k_icp_pipe launches for several templates, the whole-cluster
// launch, the persistent launch for a few clusters, and the sliced multi-launch loop for whatever is left (rule C17 on:
// k_icp_plane takes every live cluster and finishes the stage; none of the others runs).  A driver sets
// *done when it has run the stage to its end (records read back, stream synchronised); otherwise the drivers after it take
// the clusters it left and find the ones it ran finished in d_st / h_st (the stream orders them).
}  // namespace cd

namespace {
// kind: 0 = no persistent kernel can take the template, 1 = k_icp_pipe (LDS-resident, gridded), 2 = k_icp_pipe_big (global memory)
int tpl_kind(const cd_context* c, const IcpCluster& cl) {
    if (cl.tpl_m <= 0 || !c->tpl_gridded[cl.slot]) return 0;
    if (cl.tpl_m <= ICP_TPL_LDS) return 1;
    return c->tpl_big[cl.slot] ? 2 : 0;
}

struct TplGroup { int beg, end, live; int kind; long long pts; };

struct IcpPlan {   // host-side decisions of one ICP stage (plan_icp)
    int ncl = 0, guess_mode = CD_GUESS_NONE, max_n = 0, qslice = 0;
    size_t guess_need = 0;                       // floats of the guess upload
    const std::vector<float>* frame_guess = nullptr;   // per-frame guesses: cd_set_frame_guesses' or (CD_GUESS_SURFACE) the call's own
    std::vector<char> in_lat;                    // the cluster takes k_icp_lat
    int n_lat = 0, n_live = 0, lat_max_n = 0;
    std::vector<TplGroup> groups;
    int nwork = 0;                               // items of the sliced work list (h_work)
    int wg_cap = 0;                              // workgroups of a persistent ICP launch at most (CUBOID_ICP_MAX_WG)
    bool grouped_pipe = false, lat_direct = false, pipe_ok = false, big_ok = false, whole_cluster = false;
    bool pre_zeroed = false;                     // (icp_setup) d_acc / d_accf / d_queue were zeroed by the fused call
    bool crowded = false;                        // (icp_params) four or more batches in flight on the device
    bool plane = false;                          // rule C17 (cd_set_icp_plane_weight): every live cluster takes k_icp_plane
};

// Clusters h_cl[0..ncl) -> plan; fills the work list h_work, tile0 of every cluster and the initial states h_st.
int plan_icp(cd_context* c, int ncl, const cd_params* p, IcpPlan* pl) {
    pl->ncl = ncl;
    // initial guess (pcl::Registration::align(output, guess)); the default - and the reference's live path - is none
    // (CD_GUESS_SURFACE is CD_GUESS_PER_FRAME with the guesses the call derived itself)
    const int guess_mode = pl->guess_mode = p->icp_use_guess == CD_GUESS_SURFACE ? CD_GUESS_PER_FRAME : p->icp_use_guess;
    pl->frame_guess = p->icp_use_guess == CD_GUESS_SURFACE ? &c->surface_guess : &c->frame_guess;
    if (guess_mode != CD_GUESS_NONE) {
        int max_frame = 0;
        for (int k = 0; k < ncl; ++k) { pl->max_n = std::max(pl->max_n, c->h_cl[k].n); max_frame = std::max(max_frame, c->h_cl[k].frame); }
        pl->guess_need = guess_mode == CD_GUESS_PER_FRAME ? 16 * ((size_t)max_frame + 1) : (guess_mode == CD_GUESS_CLUSTER ? 16 * (size_t)ncl : 16);
        if (guess_mode == CD_GUESS_PER_FRAME && pl->frame_guess->size() < pl->guess_need) return fail(c, CD_ERR_INVALID_ARG, "icp_use_guess = CD_GUESS_PER_FRAME but cd_set_frame_guesses holds fewer frames than the batch");
    }
    // queries per workgroup: 512 when the batch fills the chip, smaller slices (more workgroups) otherwise
    long long qtot = 0;
    for (int k = 0; k < ncl; ++k) qtot += c->h_cl[k].n;
    pl->qslice = std::max(64, std::min(ICP_QSLICE, (int)((qtot / 512 + 15) / 16 * 16)));
    // Template groups: runs of clusters that share a template (one run per template when every cluster is matched against
    // every template).  With several templates in the batch, the groups whose template is LDS-resident and gridded go through
    // ONE k_icp_pipe launch (each group gets a share of the workgroups and its own queue) when there are enough of them to
    // fill a fifth of the chip; the other clusters take the sliced driver.
    // Clusters whose template is a lattice (every make_cuboid.py template; IcpLattice, common.hpp) go to k_icp_lat - closed-form
    // nearest neighbour, one workgroup per cluster - and take no part in the grouping.  CUBOID_ICP_LATTICE=0 and the
    // forced driver modes (CUBOID_ICP_MODE) keep them on the generic searches (A/B, and the GPU suite runs under each mode).
    // Rule C17 on: every live cluster goes to k_icp_plane whatever those switches say - no other driver implements the step.
    pl->plane = c->plane_weight != 0.0;
    const bool use_lat = !pl->plane && c->tun.icp_lattice != 0 && c->tun.icp_mode == 0;
    pl->in_lat.assign((size_t)ncl, 0);
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = c->h_cl[k];
        const bool live = cl.n >= 3 && cl.tpl_m > 0;
        pl->n_live += live ? 1 : 0;
        if (pl->plane && live && c->tpl_faces[cl.slot] <= 0) return fail(c, CD_ERR_INVALID_ARG, "plane-weighted ICP is on and a template of the call is not a lattice");
        if (use_lat && live && c->tpl_faces[cl.slot] > 0) { pl->in_lat[(size_t)k] = 1; ++pl->n_lat; pl->lat_max_n = std::max(pl->lat_max_n, cl.n); }
    }
    c->timing.icp_search = pl->plane ? 1 : (pl->n_lat == 0 ? 0 : (pl->n_lat == pl->n_live ? 1 : 2));
    std::vector<TplGroup>& groups = pl->groups;
    for (int k = 0; k < ncl; ++k) {
        const IcpCluster& cl = c->h_cl[k];
        if (groups.empty() || c->h_cl[groups.back().beg].tpl_off != cl.tpl_off || c->h_cl[groups.back().beg].tpl_m != cl.tpl_m)
            groups.push_back(TplGroup{k, k, 0, use_lat && c->tpl_faces[cl.slot] > 0 ? 0 : tpl_kind(c, cl), 0});
        TplGroup& g = groups.back();
        g.end = k + 1;
        if (cl.n >= 3) { g.live += 1; g.pts += cl.n; }
    }
    int n_grouped = 0;
    for (const TplGroup& g : groups) if (g.kind) n_grouped += g.live;
    pl->grouped_pipe = !pl->plane && groups.size() > 1 && groups.size() <= 16 && n_grouped > 0 &&
                       (c->tun.icp_mode == 3 || (c->tun.icp_mode == 0 && n_grouped * 5 >= c->n_cu));
    if (std::getenv("CUBOID_DEBUG")) {
        std::fprintf(stderr, "cuboid_hip: stage_icp %d clusters, %zu template groups, %d in pipe groups, grouped_pipe %d:", ncl, groups.size(), n_grouped, (int)pl->grouped_pipe);
        for (const TplGroup& g : groups) std::fprintf(stderr, " [%d,%d) m=%d kind=%d live=%d", g.beg, g.end, c->h_cl[g.beg].tpl_m, g.kind, g.live);
        std::fprintf(stderr, "\n");
    }
    std::vector<char> in_pipe((size_t)ncl, 0);
    if (pl->grouped_pipe)
        for (const TplGroup& g : groups) if (g.kind) for (int k = g.beg; k < g.end; ++k) in_pipe[(size_t)k] = 1;
    int nwork = 0;
    for (int k = 0; k < ncl; ++k) {
        IcpCluster& cl = c->h_cl[k];
        cl.tile0 = nwork;
        const int tiles = cl.n >= 3 && cl.tpl_m > 0 && !in_pipe[(size_t)k] && !pl->in_lat[(size_t)k] && !pl->plane ? (cl.n + pl->qslice - 1) / pl->qslice : 0;
        if (nwork + tiles > c->work_cap) return fail(c, CD_ERR_CAPACITY, "ICP work list overflow");
        for (int t = 0; t < tiles; ++t) c->h_work[nwork++] = IcpWork{k, t};
        for (int s = 0; s < 2; ++s) {
            IcpState& st = c->h_st[2 * k + s];
            std::memset(&st, 0, sizeof(st));
            for (int i = 0; i < 4; ++i) st.Tfinal[5 * i] = 1.f;
            if (guess_mode != CD_GUESS_NONE && guess_mode != CD_GUESS_CLUSTER)   // final_transformation_ = guess (CD_GUESS_CLUSTER: k_shape_frames writes it on the device)
                std::memcpy(st.Tfinal, guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess->data() + 16 * (size_t)cl.frame : p->icp_guess, 64);
            st.prev_mse = std::numeric_limits<double>::max();
            if (cl.tpl_m <= 0) { st.done = 1; st.status = CD_ERR_NO_TEMPLATE; }
            else if (cl.n < 3) { st.done = 1; st.status = CD_ERR_FEW_CORRESPONDENCES; }
        }
    }
    pl->nwork = nwork;
    pl->wg_cap = c->tun.icp_max_wg > 0 ? std::min(c->tun.icp_max_wg, c->n_cu) : c->n_cu;
    // A stage whose clusters ALL take k_icp_lat (the default template, no initial guess): the kernel reads the cluster list, the
    // order and the initial states from the pinned host arrays and writes the final states and fitness sums there - a few
    // hundred bytes per cluster once at each end of its ICP - instead of three copy launches around it.
    pl->lat_direct = c->tun.icp_direct && pl->n_lat > 0 && pl->n_lat == pl->n_live && guess_mode == CD_GUESS_NONE && c->tun.mirror_reads && c->tun.mirror_writes && c->tun.copy_kernels;
    // Batch mode: with at least ~n_cu/5 clusters every CU can own whole clusters, so each cluster runs its
    // complete ICP (all iterations + fitness) inside one persistent workgroup, one launch for the batch.
    // The pipelined variant (two to four clusters in flight per workgroup, no barrier in the iteration loop) needs one
    // LDS-resident gridded template shared by every cluster of the launch; otherwise k_icp_cluster runs.
    bool one_tpl = true;
    for (int k = 1; k < ncl && one_tpl; ++k) one_tpl = c->h_cl[k].tpl_off == c->h_cl[0].tpl_off && c->h_cl[k].tpl_m == c->h_cl[0].tpl_m;
    pl->pipe_ok = c->tun.icp_mode != 2 && one_tpl && tpl_kind(c, c->h_cl[0]) == 1;
    // ... or, for a template that does not fit LDS, its twin that reads the template from global memory (k_icp_pipe_big)
    pl->big_ok = c->tun.icp_mode != 2 && one_tpl && tpl_kind(c, c->h_cl[0]) == 2;
    // (auto mode: only the pipelined kernel beats the sliced driver; with mixed or non-resident templates k_icp_cluster's
    // barrier per iteration costs more than it saves, so those batches stay sliced unless the mode is forced)
    // (measured crossover on the bench frames: 33 clusters 3.3 ms sliced / 3.7 ms pipelined, 65 clusters 4.4 / 3.9, 130 clusters
    // 6.4 / 4.0: the pipelined kernel wins from about a fifth of the CUs' worth of clusters)
    pl->whole_cluster = !pl->grouped_pipe && (c->tun.icp_mode >= 2 || (c->tun.icp_mode == 0 && ncl * 5 >= c->n_cu && (pl->pipe_ok || pl->big_ok)));
    return CD_OK;
}

// which guess k_icp_apply_guess moves problem k by: the only one, its frame's, its own
int guess_indexing(int guess_mode) { return guess_mode == CD_GUESS_PER_FRAME ? 1 : (guess_mode == CD_GUESS_CLUSTER ? 2 : 0); }


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

// the stream operations every driver needs before the stage's start event: guess, cluster list, work list, initial states,
// zeroed sums, guess applied to the sources
int icp_setup(cd_context* c, const cd_params* p, IcpPlan* pl) {
    const int ncl = pl->ncl;
    if (pl->guess_mode != CD_GUESS_NONE) {
        GROW(c, d_guess, pl->guess_need);
        if (pl->guess_mode == CD_GUESS_CLUSTER) {   // (the guesses are written on the device; the records' buffers before anything is on the stream)
            GROW(c, d_shape, (size_t)ncl); GROW(c, h_shape, (size_t)ncl);
            GROW(c, d_tframe, (size_t)CD_MAX_TEMPLATES); GROW(c, h_tframe, (size_t)CD_MAX_TEMPLATES);
        } else
            HIPCHK(c, copy_sync(c, c->d_guess, pl->guess_mode == CD_GUESS_PER_FRAME ? pl->frame_guess->data() : p->icp_guess, sizeof(float) * pl->guess_need, hipMemcpyHostToDevice));
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
    if (c->icp_bounded) {   // rule C8: the sliced / persistent drivers' correspondence counts, [cluster][it % 3]
        GROW(c, d_ncorr, 3 * (size_t)ncl);
        HIPCHK(c, hipMemsetAsync(c->d_ncorr, 0, sizeof(uint32_t) * 3 * (size_t)ncl, c->stream));
    }
    if (pl->guess_mode == CD_GUESS_CLUSTER) {   // rule C13: record, guess and Tfinal of every problem, after the d_cl / d_st upload above
        if (int e = launch_cluster_guesses(c, ncl)) return e;
        HIPCHK(c, xfer(c, c->h_shape, c->d_shape, sizeof(ShapeFrame) * (size_t)ncl, hipMemcpyDeviceToHost));   // (on the host by the stage's final synchronisation)
    }
    if (pl->guess_mode != CD_GUESS_NONE)   // input_transformed = guess * source (d_src is a copy of d_src0 at this point)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl->max_n, c->d_cl, c->d_guess, guess_indexing(pl->guess_mode), c->d_src0, c->d_src));
    return CD_OK;
}

IcpParams icp_params(const cd_context* c, const cd_params* p, bool* crowded) {
    IcpParams ip;
    ip.max_iter = p->icp_max_iterations;
    ip.grid_rc = 1.0f;
    if (const char* e = std::getenv("CUBOID_ICP_GRID_RC")) ip.grid_rc = (float)std::atof(e);
    ip.trans_eps = p->icp_transformation_epsilon;
    ip.rel_mse = p->icp_euclidean_fitness_epsilon;
    ip.rot_thr = 1.0 - p->icp_transformation_epsilon;
    ip.abs_mse = 1e-12;
    // Whole-cluster launches: how many clusters a workgroup keeps in flight and how many workgroups there are.  A call that has
    // the device to itself wants every CU at work: one workgroup per CU (or per cluster), two slots, the second filled as long
    // as clusters are left.  With other calls in flight (BatchPipeline) the chip is full anyway and what counts is the CU-time
    // a batch costs: FOUR clusters per workgroup keep its sixteen waves supplied while one of them solves a step (no wave waits
    // at a hand-over, no workgroup ends with one cluster alone), on a quarter as many workgroups - the other batches have the
    // other CUs (config 3, 522 clusters: 2 x 256 -> 4 x 128 is 48.4 -> 53.3 k frames/s; grids that are not a multiple of 32 -
    // 4 per XCD and shader engine - lose 2-4 %).
    // (crossover measured on config 3: with two calls in flight the two shapes tie, with three 2 x 256 wins 49.4 : 46.5 k, with
    // four 4 x 128 wins 52.9 : 49.7 k - and the last launches of a burst, which soon have the GPU to themselves, spread out)
    *crowded = device_shared(c).batches_in_flight.load() >= 4;
    ip.pipe_slots = c->tun.icp_slots > 0 ? std::min(c->tun.icp_slots, CD_PIPE_SLOTS) : (*crowded ? CD_PIPE_SLOTS : std::min(2, CD_PIPE_SLOTS));
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
int icp_run_lat(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, n_lat = pl.n_lat, lat_max_n = pl.lat_max_n;
    // the clusters of the launch, largest first
    int no = 0;
    for (int k = 0; k < ncl; ++k) if (pl.in_lat[(size_t)k]) c->h_order[no++] = k;
    std::stable_sort(c->h_order.get(), c->h_order + no, [&](int a, int b) { return c->h_cl[a].n > c->h_cl[b].n; });
    if (!pl.lat_direct) HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    // Shape of the launch (k_icp_lat.hip): clusters per workgroup x waves per cluster.  A call that has the GPU to itself wants
    // the launch short: one cluster per workgroup, four waves each when there are clusters enough to fill the chip twice that way,
    // eight or sixteen for fewer or very large clusters (one frame; config 5's thousands of points).  With other batches in
    // flight the chip is full anyway: four clusters per workgroup, two waves each, pay the single-lane solve of a round once
    // for the four (measured on config 3, seven in flight, profiles/r05_lat_shapes.txt: 1x4 145-146 k, 4x2 149-151 k, 8x2 146 k,
    // 4x4 139 k, 4x1 131 k frames/s; alone 1x4 1.34 ms, 1x8 1.30, 4x2 2.2, 4x1 2.8).  CUBOID_LAT_SHAPE=cpw,wpc[,clusters per slot].
    const bool busy = device_shared(c).batches_in_flight.load() >= 3;
    int cpw = 1, wpc = n_lat >= 768 ? 4 : (n_lat >= 96 ? 8 : 16), per_slot = 1;   // (end of round 5, 522 clusters alone: 1x4 1.17 ms, 1x8 1.10, 1x16 1.53, 2x4 1.27)
    if (lat_max_n > 16384) wpc = 16;
    else if (lat_max_n > 4096) wpc = std::max(wpc, 8);
    if (busy && n_lat >= 256 && lat_max_n <= 8192) { cpw = 4; wpc = 2; }
    if (c->tun.lat_shape[0] > 0) { cpw = c->tun.lat_shape[0]; wpc = std::max(1, c->tun.lat_shape[1]); per_slot = std::max(1, c->tun.lat_shape[2]); }
    const int n_wg = std::max(1, (n_lat + cpw * per_slot - 1) / (cpw * per_slot));
    GateHold lat_hold;   // (CUBOID_ICP_CONCURRENT: at most that many contexts between this launch and its completion)
    if (c->tun.icp_concurrent > 0) lat_hold.enter(&device_shared(c).icp_gate, c->tun.icp_concurrent);
    if (!pl.pre_zeroed) HIPCHK(c, hipMemsetAsync(c->d_queue, 0, 2 * sizeof(int), c->stream));   // head of the cluster queue, count of finished workgroups
    if (pl.lat_direct) std::memset(c->h_accf, 0, sizeof(unsigned long long) * ((size_t)ncl + 1));   // (what the zeroed device array used to bring back for clusters the kernel skips)
    if (pl.lat_direct)
        LAUNCH(c, launch_icp_lat(c->stream, n_lat, cpw, wpc, n_wg, c->h_order, c->h_cl, c->h_st, c->h_accf, c->d_lat, c->d_src, c->d_src0, c->d_queue, c->d_accf + ncl, c->h_accf + ncl, ip, icp_bound(c)));
    else
        LAUNCH(c, launch_icp_lat(c->stream, n_lat, cpw, wpc, n_wg, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_lat, c->d_src, c->d_src0, c->d_queue, c->d_accf + ncl, nullptr, ip, icp_bound(c)));
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (cpw << 16) | std::min(n_wg, 0xffff);
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
int icp_run_plane(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    static_assert(sizeof(PlaneStats) == sizeof(cd_icp_plane_stats), "PlaneStats mirrors cd_icp_plane_stats");
    const int ncl = pl.ncl;
    int no = 0;
    for (int k = 0; k < ncl; ++k) if (c->h_cl[k].n >= 3 && c->h_cl[k].tpl_m > 0) c->h_order[no++] = k;
    std::stable_sort(c->h_order.get(), c->h_order + no, [&](int a, int b) { return c->h_cl[a].n > c->h_cl[b].n; });
    GROW(c, d_pstat, (size_t)ncl); GROW(c, h_pstat, (size_t)ncl);
    if (no > 0) HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_pstat, 0, sizeof(PlaneStats) * (size_t)ncl, c->stream));   // (pre-marked problems keep zeros)
    if (!pl.pre_zeroed) HIPCHK(c, hipMemsetAsync(c->d_queue, 0, 2 * sizeof(int), c->stream));   // head of the cluster queue
    PlaneParams pp;
    pp.lambda = (float)c->plane_weight;
    pp.latched0 = std::isinf(c->plane_switch) ? 1 : 0;
    pp.switch2 = c->plane_switch * c->plane_switch;
    // two workgroups per CU at the most: 256 registers a wave leave two waves per SIMD (k_icp_plane.hip)
    const int n_wg = std::max(1, std::min(no, 2 * pl.wg_cap));
    LAUNCH(c, launch_icp_plane(c->stream, no, n_wg, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_pstat, c->d_lat, c->d_src, c->d_src0, c->d_queue, ip, icp_bound(c), pp));
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

// The template groups of a several-template batch (plan.grouped_pipe): k_icp_pipe and k_icp_pipe_big side by side; the stage
// is finished when no cluster is left for the sliced driver.
int icp_run_grouped(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl;
    // items of `order`: the pipe groups one after the other (those of k_icp_pipe first, then those of k_icp_pipe_big),
    // each largest cluster first.  The two kernels are launched side by side (second stream): their workgroups share the
    // chip, every group gets workgroups in proportion to its points (a query against a template in global memory
    // counted BIG_WEIGHT times), at least one, no more than it has clusters.
    const int wg_cap = pl.wg_cap;
    // (while every problem can have a workgroup of its own the launch lasts as long as its longest cluster, and those are the
    // global-memory ones: 4; with more problems than workgroups it is their throughput that counts, 1.6 x the LDS kernel's
    // cost per workgroup plus the longer tail: 2 - config 5 at 8 frames per batch 4 > 2 by 5 %, at 64 frames 2 > 4 by 6 %)
    int live_all = 0;
    for (const TplGroup& g : pl.groups) if (g.kind) live_all += g.live;
    const long long BIG_WEIGHT = c->tun.icp_big_weight > 0 ? c->tun.icp_big_weight : (live_all <= wg_cap ? 4 : 2);
    const int cpw = std::max(1, c->tun.icp_cpw);   // (0 = default: a group may have as many workgroups as clusters)
    // (template groups keep two clusters in flight per workgroup whatever the regime: every group has its share of the
    // workgroups and its own queue already, and four slots measure 3-7 % slower on config 5)
    IcpParams ipg = ip;
    if (c->tun.icp_slots <= 0) ipg.pipe_slots = std::min(2, CD_PIPE_SLOTS);
    int* tab = c->h_wgtab;   // pinned: the copy below is asynchronous
    int ntab = 0;
    long long pts_all = 0;
    int npg = 0;
    for (const TplGroup& g : pl.groups) if (g.kind && g.live > 0) { pts_all += g.pts * (g.kind == 2 ? BIG_WEIGHT : 1); ++npg; }
    int no = 0, gq = 0, n_wg = 0, wg_of[3] = {0, 0, 0}, tab_of[3] = {0, 0, 0};
    for (int kind = 1; kind <= 2; ++kind) {
        tab_of[kind] = ntab;
        for (const TplGroup& g : pl.groups) {
            if (g.kind != kind || g.live == 0) continue;
            const int b = no;
            for (int k = g.beg; k < g.end; ++k) if (c->h_cl[k].n >= 3) c->h_order[no++] = k;
            std::stable_sort(c->h_order + b, c->h_order + no, [&](int x, int y) { return c->h_cl[x].n > c->h_cl[y].n; });
            int share = (int)((long long)wg_cap * g.pts * (kind == 2 ? BIG_WEIGHT : 1) / std::max(pts_all, 1ll));
            share = std::max(1, std::min(share, std::min((g.live + cpw - 1) / cpw, wg_cap - n_wg - (npg - 1 - gq))));
            for (int w = 0; w < share && ntab + 3 <= 3 * 1024; ++w) { tab[ntab++] = b; tab[ntab++] = no; tab[ntab++] = gq; }
            n_wg += share;
            wg_of[kind] += share;
            ++gq;
        }
    }
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * (size_t)no, hipMemcpyHostToDevice));
    HIPCHK(c, xfer(c, c->d_wgtab, tab, sizeof(int) * (size_t)ntab, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int) * 16, c->stream));   // one queue head per group
    // the LDS-template launch goes to the context's stream (stream3 with icp_lowprio), the global-template launch beside it
    hipStream_t s1 = c->tun.icp_lowprio ? c->stream3 : c->stream;
    hipStream_t s2 = (c->tun.icp_lowprio || (wg_of[1] > 0 && wg_of[2] > 0)) ? c->stream2 : c->stream;
    if (s1 != c->stream || s2 != c->stream) {   // everything uploaded so far is visible to the side streams
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        if (s1 != c->stream) HIPCHK(c, hipStreamWaitEvent(s1, c->ev2[0], 0));
        if (s2 != c->stream) HIPCHK(c, hipStreamWaitEvent(s2, c->ev2[0], 0));
    }
    if (wg_of[1] > 0)
        LAUNCH(c, launch_icp_pipe(s1, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                        c->d_queue, wg_of[1], c->d_wgtab + tab_of[1], ipg, icp_bound(c)));
    if (wg_of[2] > 0)
        LAUNCH(c, launch_icp_pipe_big(s2, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tplk, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid,
                            c->d_super, c->d_tcell, c->d_src, c->d_src0, c->d_nn, c->d_queue, wg_of[2], c->d_wgtab + tab_of[2], ipg, icp_bound(c)));
    if (s1 != c->stream && wg_of[1] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[2], s1));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[2], 0));
    }
    if (s2 != c->stream && wg_of[2] > 0) {
        HIPCHK(c, hipEventRecord(c->ev2[1], s2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev2[1], 0));
    }
    c->timing.icp_kernel_launches = 1;
    c->timing.icp_regime = (ipg.pipe_slots << 16) | n_wg;
    if (pl.nwork > 0) {   // the other clusters take the sliced driver
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;
    return CD_OK;
}

// One launch in which every cluster runs its whole ICP in one workgroup (plan.whole_cluster): k_icp_pipe, k_icp_pipe_big or
// k_icp_cluster.  Always finishes the stage.
int icp_run_whole(cd_context* c, const IcpPlan& pl, IcpParams ip, bool* done) {
    const int ncl = pl.ncl;
    auto pipe_grid = [&](int n_items, int cap) {   // workgroups of the launch over n_items clusters
        if (c->tun.icp_cpw > 0) return std::min((n_items + c->tun.icp_cpw - 1) / c->tun.icp_cpw, cap);
        if (!pl.crowded || n_items <= cap) return std::min(n_items, cap);
        return std::min(cap, std::max(32, (n_items / ip.pipe_slots + 16) / 32 * 32));
    };
    GateHold hold;   // (released on every path out of this function)
    if (c->tun.icp_concurrent > 0) hold.enter(&device_shared(c).icp_gate, c->tun.icp_concurrent);
    for (int k = 0; k < ncl; ++k) c->h_order[k] = k;
    std::stable_sort(c->h_order.get(), c->h_order + ncl, [&](int a, int b) { return c->h_cl[a].n > c->h_cl[b].n; });
    HIPCHK(c, xfer(c, c->d_order, c->h_order, sizeof(int) * ncl, hipMemcpyHostToDevice));
    const int wg_cap = pl.wg_cap;
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int), c->stream));   // head of the cluster queue
    hipStream_t si = c->tun.icp_lowprio >= 2 ? c->stream3 : c->stream;
    if (pl.pipe_ok || pl.big_ok) {
        c->timing.icp_regime = (ip.pipe_slots << 16) | pipe_grid(ncl, wg_cap);
        // A launch that has the GPU to itself lets workgroups that run out of clusters wait and take over running ones
        // (k_icp.hip, "hand-over of running clusters"): the launch is as long as its slowest workgroup, and the bench batch's
        // slowest runs 25 % over the average.  With other calls in flight a waiting workgroup would sit on a CU their
        // kernels could use, and what counts there is the CU-time a batch costs, which hand-overs do not lower.
        const bool alone = device_shared(c).batches_in_flight.load() <= 1;
        ip.donate = (c->tun.icp_donate < 0 ? (alone && ncl > pipe_grid(ncl, wg_cap)) : c->tun.icp_donate != 0) ? 1 : 0;
        if (ip.donate) HIPCHK(c, hipMemsetAsync(c->d_don, 0, sizeof(int) * (size_t)(DON_BOX + DON_CAP), c->stream));
    }
    if (si != c->stream) {   // (after the control block was zeroed on c->stream: the launch on `si` must see it zeroed - ADVICE r4)
        HIPCHK(c, hipEventRecord(c->ev2[0], c->stream));
        HIPCHK(c, hipStreamWaitEvent(si, c->ev2[0], 0));
    }
    if (pl.pipe_ok)
        LAUNCH(c, launch_icp_pipe(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                        c->d_queue, pipe_grid(ncl, wg_cap), nullptr, ip, icp_bound(c)));
    else if (pl.big_ok)
        LAUNCH(c, launch_icp_pipe_big(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tplk, c->d_tlok, c->d_thik, c->d_kdmap, c->d_grid, c->d_super, c->d_tcell,
                            c->d_src, c->d_src0, c->d_nn, c->d_queue, pipe_grid(ncl, wg_cap), nullptr, ip, icp_bound(c)));
    else
        LAUNCH(c, launch_icp_cluster(si, ncl, c->d_order, c->d_cl, c->d_st, c->d_accf, c->d_tpl, c->d_tlo, c->d_thi, c->d_grid, c->d_tcell, c->d_src, c->d_src0, c->d_nn,
                           c->d_queue, wg_cap, ip, icp_bound(c)));
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
// iteration instead of two kernel launches).  Needs all its workgroups resident together; a barrier that does not
// complete in time makes it give up, and the sliced driver takes over from the initial state (not done).
int icp_run_persist(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, nwork = pl.nwork;
    // (with other contexts at work - BatchPipeline - their persistent kernels hold the CUs this launch's grid barrier needs:
    // it would wait, give up and hand over; go straight to the multi-launch loop then)
    const bool siblings = device_shared(c).calls_in_flight.load() > 1;
    if (nwork == 0 || !c->tun.icp_persist || (siblings && c->tun.icp_persist != 2)) return CD_OK;
    const int G = std::min(nwork, pl.wg_cap);
    // measured against the multi-launch loop: 1 frame 1.50 / 1.78 ms, 4 frames 1.94 / 2.36, 8 frames 3.04 / 2.66 - with many
    // clusters the launch lasts as long as the slowest one while finished workgroups wait at the barriers, and a workgroup
    // with several items solves for each of them in turn
    if (ncl > 8 || nwork > G) return CD_OK;
    int n_open = 0;
    for (int k = 0; k < ncl; ++k) if (c->h_cl[k].tile0 < (k + 1 < ncl ? c->h_cl[k + 1].tile0 : nwork)) ++n_open;
    // d_queue[4] barrier counter, [5] abort flag, [6..9] clusters closed per iteration slot (k_icp_persist's exit test)
    int* ctl = c->h_ctl;
    for (int i = 0; i < 8; ++i) ctl[i] = 0;
    ctl[1] = c->tun.icp_persist == 2 ? 1 : 0;
    HIPCHK(c, xfer(c, c->d_queue + 4, ctl, sizeof(int) * 6, hipMemcpyHostToDevice));
    LAUNCH(c, launch_icp_persist(c->stream, nwork, G, ip.max_iter + 3, c->d_work, c->d_cl, c->d_st, c->d_acc, c->d_accf, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid,
                       c->d_src, c->d_src0, c->d_nn, c->d_d2, pl.qslice, (unsigned*)(c->d_queue + 4), c->d_queue + 5, n_open, c->d_queue + 6, ip, icp_bound(c)));
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, xfer(c, ctl + 8, c->d_queue + 5, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    c->st_init.assign(c->h_st.get(), c->h_st + 2 * (size_t)ncl);   // in case the launch gives up (no reallocation after the first call)
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
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
    if (pl.guess_mode != CD_GUESS_NONE)
        LAUNCH(c, launch_icp_apply_guess(c->stream, ncl, pl.max_n, c->d_cl, c->d_guess, guess_indexing(pl.guess_mode), c->d_src0, c->d_src));
    return CD_OK;
}

// The multi-launch loop over the work list, then the fitness pass.  Always finishes the stage.
int icp_run_sliced(cd_context* c, const IcpPlan& pl, const IcpParams& ip, bool* done) {
    const int ncl = pl.ncl, nwork = pl.nwork, max_launch = ip.max_iter + 3;
    // The iteration kernel walks an ACTIVE work list (d_work2) that the host re-packs at every
    // completion poll, dropping the clusters that have converged; the full list (d_work) is kept for
    // the fitness pass.  A cluster whose state shows done in either parity slot has already had its
    // final transform applied, so it needs no further work items (k_icp_solve alone keeps its state).
    int it = 0, nactive = nwork;
    std::memcpy(c->h_work2, c->h_work, sizeof(IcpWork) * (size_t)std::max(nwork, 1));
    HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)std::max(nwork, 1), hipMemcpyHostToDevice));
    int group = 8;
    while (nwork > 0 && it < max_launch) {
        const int g = std::min(group, max_launch - it);
        for (int q = 0; q < g; ++q) LAUNCH(c, launch_icp_iter(c->stream, it++, nactive, ncl, c->d_work2, c->d_cl, c->d_st, c->d_acc, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid, c->d_src, c->d_nn, c->d_d2, pl.qslice, c->d_queue, c->n_cu, ip, icp_bound(c)));
        HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool all = true;
        int na = 0;
        for (int w = 0; w < nwork; ++w) {
            const int k = c->h_work[w].cluster;
            if (!(c->h_st[2 * k].done || c->h_st[2 * k + 1].done)) c->h_work2[na++] = c->h_work[w];
        }
        for (int k = 0; k < ncl && all; ++k) all = c->h_st[2 * k].done && c->h_st[2 * k + 1].done;
        if (all) break;
        if (na != nactive) {
            nactive = na;
            if (na > 0) HIPCHK(c, xfer(c, c->d_work2, c->h_work2, sizeof(IcpWork) * (size_t)na, hipMemcpyHostToDevice));
        }
        group = 16;
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));   // (before the fitness pass)
    c->timing.icp_kernel_launches = it;
    LAUNCH(c, launch_icp_fitness(c->stream, nwork, c->d_work, c->d_cl, c->d_st, 0, c->d_accf, c->d_tplk, c->d_tlok, c->d_thik, c->d_grid, c->d_src0, c->d_nn, c->d_d2, pl.qslice));
    HIPCHK(c, xfer(c, c->h_accf, c->d_accf, sizeof(unsigned long long) * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, xfer(c, c->h_st, c->d_st, sizeof(IcpState) * 2 * ncl, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *done = true;
    return CD_OK;
}

}  // namespace

namespace cd {
// S6.  clusters described by h_cl[0..ncl) (src_off relative to d_src/d_src0).  Fills h_st / h_accf.
int stage_icp(cd_context* c, int ncl, const cd_params* p, long long* pair_tests) {
    c->timing.icp_kernel_launches = 0;
    c->timing.icp_kernel_ms = 0.f;
    if (pair_tests) *pair_tests = 0;
    if (ncl <= 0) return CD_OK;
    IcpPlan pl;
    int st = plan_icp(c, ncl, p, &pl);
    if (!st) st = icp_setup(c, p, &pl);
    if (st) return st;
    const IcpParams ip = icp_params(c, p, &pl.crowded);
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    bool done = false;
    if (pl.plane) st = icp_run_plane(c, pl, ip, &done);
    if (!st && !done && pl.n_lat > 0) st = icp_run_lat(c, pl, ip, &done);
    if (!st && !done && pl.grouped_pipe) st = icp_run_grouped(c, pl, ip, &done);
    if (!st && !done && pl.whole_cluster) st = icp_run_whole(c, pl, ip, &done);
    if (!st && !done) st = icp_run_persist(c, pl, ip, &done);
    if (!st && !done) st = icp_run_sliced(c, pl, ip, &done);
    if (done) icp_finish(c, ncl, pair_tests);
    return st;
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
