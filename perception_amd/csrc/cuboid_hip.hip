// cuboid_hip.hip - the front-end stage drivers of the pipeline, device-resident in and out: S0 .. S5 (crop + voxel grid, plane,
// extract, cluster) and the records they hand to S6 (icp_stage.hip).  The fused call (batch.hip) and the entries (entries.hip) run them.
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
// fs.status updated for NO_MODEL, iterations per frame; plane_gave_up[f] = 1 (and h_have[f] = 0, cd_last_error set) for a frame
// whose sampler ran into a device limit before PCL's loop ended - the callers report CD_ERR_CAPACITY for it.
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
    c->plane_gave_up.assign((size_t)F, 0);
    for (int f = 0; f < F; ++f) c->h_active[f] = (c->h_fs[f].status == CD_OK || c->h_fs[f].status == CD_ERR_NO_MODEL) ? 1 : 0;
    ZERO_FILL(c, c->d_counts, sizeof(int) * (size_t)F * MAX_HYP);
    const int targets[4] = {16, 64, 256, MAX_HYP};
    // max_iterations + 1 hypotheses end PCL's loop; the 39 more are head-room for hypotheses marked invalid ("skipped models"),
    // which never happens: computeModelCoefficients repeats isSampleGood's comparison on the same floats, so a sample that
    // passed the one is never collinear for the other, and valid[] is 1 for every hypothesis the sampler emits
    const int h_cap = std::min(MAX_HYP, p->plane_max_iterations + 40);
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
            // (a sampler that GAVE UP on a device limit ends the frame only if PCL's loop ends within what it drew: see below)
            const bool gave_up = s.sampler_exhausted == SAMPLER_GAVE_UP;
            bool fin = rep[f].consume(c->h_counts + (size_t)f * MAX_HYP, c->h_valid + (size_t)f * MAX_HYP, s.n_hyp, std::max(1, s.n_v),
                                      p->plane_max_iterations, p->plane_probability, !gave_up && (s.sampler_exhausted != 0 || h_target >= h_cap));
            if (!fin && gave_up) {
                // PCL's loop asks for a hypothesis the device cannot draw (PCL has no such limit and would run on): no silent
                // "best model so far" - the frame fails with CD_ERR_CAPACITY and goes on as a frame without a model
                c->plane_gave_up[(size_t)f] = 1;
                std::snprintf(c->err, sizeof(c->err), "RANSAC sampler: frame %d needs hypothesis %d, beyond the device's limits (%d random draws, %d shuffle slots)",
                              f, s.n_hyp, RND_TABLE, (SAMPLER_MAP * 3) / 4);
                rep[f].best_h = -1;
                fin = true;
            }
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
}  // namespace cd
