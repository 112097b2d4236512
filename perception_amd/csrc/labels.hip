// labels.hip - point labels (rule C15, k_labels.hip): the label calls on the last fused call and the tint of label images
#include "context.hpp"
#include "host_math.hpp"
#include "label_math.hpp"

namespace {
static_assert(sizeof(cd_label_palette) == 1024 && sizeof(LabelPalette) == sizeof(cd_label_palette), "the kernel's palette is cd_label_palette");

// the eight cluster colours of the default palette, repeated with the rank
const uint8_t CLUSTER_RGB[8][3] = {{230, 25, 75}, {60, 180, 75}, {0, 130, 200}, {255, 225, 25}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230}, {170, 110, 40}};

void default_palette(cd_label_palette* p) {
    std::memset(p, 0, sizeof(*p));   // (CD_LABEL_INVALID, CD_LABEL_CROPPED and the reserved values: alpha 0)
    const uint8_t plane[4] = {128, 128, 128, 96}, object[4] = {255, 165, 0, 128}, gated[4] = {139, 0, 0, 128};
    std::memcpy(p->rgba[CD_LABEL_PLANE], plane, 4);
    std::memcpy(p->rgba[CD_LABEL_OBJECT], object, 4);
    std::memcpy(p->rgba[CD_LABEL_GATED], gated, 4);
    for (int r = 0; CD_LABEL_CLUSTER0 + r < 256; ++r) {
        std::memcpy(p->rgba[CD_LABEL_CLUSTER0 + r], CLUSTER_RGB[r % 8], 3);
        p->rgba[CD_LABEL_CLUSTER0 + r][3] = 160;
    }
}

// The three steps of k_labels.hip on the context's stream.  records (stride bytes each) or depth are device memory; so is d_out.
int stage_labels(cd_context* c, const void* d_records, size_t stride, const uint16_t* d_depth, const cd_depth_camera* cam, uint8_t* d_out) {
    const LastCall& lc = c->last_call;
    const int F = lc.F;
    int max_nv = 0;
    for (int f = 0; f < F; ++f) max_nv = std::max(max_nv, c->last_nv[(size_t)f]);
    const int vpitch = (std::max(max_nv, 1) + 63) & ~63;
    GROW(c, d_vkey, (size_t)F * vpitch);
    GROW(c, d_vclass, (size_t)F * vpitch);
    const cd_params* p = &lc.prm;
    LAUNCH(c, launch_label_voxel_keys(c->stream, c->d_key[lc.keys.cur], c->N, F, c->d_fs, lc.keys.by_runs, c->d_vkey, vpitch));
    const ExtractArgs ea = extract_args(p, -1);
    const float4* model_p = c->tun.mirror_reads ? c->h_model : c->d_model;   // (as stage_extract read them: nothing has written them since)
    const int* have_p = c->tun.mirror_reads ? c->h_active : c->d_have;
    LAUNCH(c, launch_label_voxel_classes(c->stream, c->d_vox, c->N, F, c->d_fs, model_p, have_p, ea.thr, p->extract_negative, p->crop2_enable, ea.z2lo, ea.z2hi,
                                         ea.gate, lc.rects, c->d_plane_idx, c->d_label, c->d_vclass, vpitch,
                                         lc.prism      ? OutlierMap{c->d_pmap, c->d_plrec, lc.omap_pitch}   // (rule C20: its map, composed with the filter's when both ran)
                                         : lc.filtered ? OutlierMap{c->d_omap, c->d_orec, lc.omap_pitch}
                                                       : OutlierMap{nullptr, nullptr, 0}));
    LabelPointsParams lp;
    std::memset(&lp, 0, sizeof(lp));
    lp.lim.zlo = hm::fold_ge(p->crop_z_min); lp.lim.zhi = hm::fold_le(p->crop_z_max);
    lp.lim.xlo = hm::fold_ge(p->crop_x_min); lp.lim.xhi = hm::fold_le(p->crop_x_max);
    lp.inv_leaf = 1.0f / p->leaf_size;
    lp.packed = lc.keys.packed;
    lp.kp = lc.keys.kp;
    lp.P = (uint32_t)lc.N;
    lp.F = F;
    lp.vpitch = vpitch;
    lp.width = cam ? (uint32_t)cam->width : 1u;
    if (cam) { lp.fx = cam->fx; lp.fy = cam->fy; lp.cx = cam->cx; lp.cy = cam->cy; lp.depth_scale = cam->depth_scale; }
    LAUNCH(c, launch_label_points(c->stream, d_records, stride, d_depth, lp, c->d_fs, c->d_vkey, c->d_vclass, d_out));
    return CD_OK;
}

// the validity rule of cd_get_cluster_results, and the shape of the call
int check_last(cd_context* c, int points_per_frame, int n_frames, size_t stride, const void* in, const void* out) {
    if (!in || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (c->last_first.size() < 2 || !c->last_clouds)
        return fail(c, CD_ERR_INVALID_ARG, "no fused call to label: none has run, or another compute call has run since");
    const LastCall& lc = c->last_call;
    if ((int)c->last_first.size() - 1 != lc.F || (int)c->last_nv.size() != lc.F) return fail(c, CD_ERR_INVALID_ARG, "no fused call to label");
    if (n_frames != lc.F || points_per_frame != lc.N) return fail(c, CD_ERR_INVALID_ARG, "n_frames and points_per_frame must be those of the fused call");
    if (stride && stride != lc.stride) return fail(c, CD_ERR_INVALID_ARG, "stride_bytes must be that of the fused call (16 for a depth-fed call)");
    if (lc.keys.cur < 0 || lc.keys.cur > 1) {
        std::snprintf(c->err, sizeof(c->err), "the voxel stage's path (%s) left no sorted keys to label from", lc.keys.path);
        return CD_ERR_INVALID_ARG;
    }
    return CD_OK;
}

// host forms: labels of the batch into d_plabel, then home
int labels_home(cd_context* c, uint8_t* out, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(out, c->d_plabel, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CD_OK;
}

int label_points_impl(cd_context* c, const void* frames, size_t stride, int points_per_frame, int n_frames, uint8_t* out, bool on_device) {
    int st = check_last(c, points_per_frame, n_frames, stride, frames, out);
    if (st) return st;
    if (stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad stride");
    const size_t total = (size_t)points_per_frame * n_frames;
    if (on_device) {
        st = stage_labels(c, frames, stride, nullptr, nullptr, out);
        if (st) return st;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    st = ensure_input(c, total * stride);
    if (st) return st;
    GROW(c, d_plabel, total);
    HIPCHK(c, hipMemcpyAsync(c->d_in, frames, total * stride, hipMemcpyHostToDevice, c->stream));
    st = stage_labels(c, c->d_in, stride, nullptr, nullptr, c->d_plabel);
    return st ? st : labels_home(c, out, total);
}

int label_depth_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, uint8_t* out, bool on_device) {
    if (!cam) return fail(c, CD_ERR_INVALID_ARG, "depth camera is NULL");
    for (float v : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(v) && v > 0.f)) return fail(c, CD_ERR_INVALID_ARG, "fx, fy and depth_scale must be finite and > 0");
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    int st = check_last(c, cam->width * cam->height, n_frames, 0, depth, out);
    if (st) return st;
    if (!c->last_call.depth_is_c7)
        return fail(c, CD_ERR_INVALID_ARG, "the fused call was a mapped call that dropped its untextured points (CD_NOTEX_DROP): its records are not the rule-C7 cloud of the depth images; label it with cd_label_points_last");
    const size_t total = (size_t)cam->width * cam->height * n_frames;
    if (on_device) {
        st = stage_labels(c, nullptr, 0, depth, cam, out);
        if (st) return st;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    GROW(c, d_vdepth, total);   // (the verify calls' upload buffer: nothing of a fused call lives there)
    GROW(c, d_plabel, total);
    HIPCHK(c, hipMemcpyAsync(c->d_vdepth, depth, total * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    st = stage_labels(c, nullptr, 0, c->d_vdepth, cam, c->d_plabel);
    return st ? st : labels_home(c, out, total);
}

int tint_impl(cd_context* c, uint8_t* rgb8, const uint8_t* labels, int width, int height, int n_frames, const cd_label_palette* palette, bool on_device) {
    if (!rgb8 || !labels) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (width <= 0 || height <= 0 || (long long)width * height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    cd_label_palette def;
    if (!palette) { default_palette(&def); palette = &def; }
    LabelPalette pal;
    std::memcpy(&pal, palette, sizeof(pal));
    const size_t px = (size_t)width * height * n_frames;
    if (on_device) {
        LAUNCH(c, launch_tint_labels(c->stream, rgb8, labels, px, pal));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CD_OK;
    }
    GROW(c, d_color, (size_t)c->N * c->F * 3);   // (sized as every other user of d_color sizes it)
    GROW(c, d_tlabel, px);
    HIPCHK(c, hipMemcpyAsync(c->d_color, rgb8, px * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_tlabel, labels, px, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, launch_tint_labels(c->stream, c->d_color, c->d_tlabel, px, pal));
    HIPCHK(c, hipMemcpyAsync(rgb8, c->d_color, px * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CD_OK;
}
}  // namespace

extern "C" {
void cd_default_label_palette(cd_label_palette* palette) {
    if (palette) default_palette(palette);
}
int cd_label_struct_size(int which) { return which == 0 ? (int)sizeof(cd_label_palette) : -1; }

int cd_label_points_last(cd_context* c, const void* frames, size_t stride_bytes, int points_per_frame, int n_frames, uint8_t* out) {
    return with_scan_retry(c, [&] { return label_points_impl(c, frames, stride_bytes, points_per_frame, n_frames, out, false); });
}
int cd_label_points_last_device(cd_context* c, const void* d_frames, size_t stride_bytes, int points_per_frame, int n_frames, uint8_t* d_out) {
    return with_scan_retry(c, [&] { return label_points_impl(c, d_frames, stride_bytes, points_per_frame, n_frames, d_out, true); });
}
int cd_label_depth_last(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, uint8_t* out) {
    return with_scan_retry(c, [&] { return label_depth_impl(c, cam, depth, n_frames, out, false); });
}
int cd_label_depth_last_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, int n_frames, uint8_t* d_out) {
    return with_scan_retry(c, [&] { return label_depth_impl(c, cam, d_depth, n_frames, d_out, true); });
}
int cd_tint_labels_batch(cd_context* c, uint8_t* rgb8, const uint8_t* labels, int width, int height, int n_frames, const cd_label_palette* palette) {
    return with_scan_retry(c, [&] { return tint_impl(c, rgb8, labels, width, height, n_frames, palette, false); });
}
int cd_tint_labels_batch_device(cd_context* c, uint8_t* d_rgb8, const uint8_t* d_labels, int width, int height, int n_frames, const cd_label_palette* palette) {
    return with_scan_retry(c, [&] { return tint_impl(c, d_rgb8, d_labels, width, height, n_frames, palette, true); });
}
}  // extern "C"
