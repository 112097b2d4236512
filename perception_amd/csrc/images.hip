// images.hip - depth to cloud (rules C7, C12), colour gate (C10), overlay (C11), pose verification (C14); the depth checks and uploads
#include "context.hpp"
#include "overlay_math.hpp"
#include "texture_math.hpp"
#include "verify_math.hpp"

namespace cd {
static TextureParams texture_params(const cd_depth_camera* cam, const cd_color_camera* cc) {
    TextureParams tp;
    tp.fx = cam->fx; tp.fy = cam->fy; tp.cx = cam->cx; tp.cy = cam->cy; tp.depth_scale = cam->depth_scale;
    tp.cfx = cc->fx; tp.cfy = cc->fy; tp.ccx = cc->cx; tp.ccy = cc->cy;
    for (int i = 0; i < 9; ++i) tp.R[i] = cc->R[i];
    for (int i = 0; i < 3; ++i) tp.t[i] = cc->t[i];
    tp.cw = cc->width; tp.ch = cc->height;
    tp.keep = cc->no_texture == CD_NOTEX_KEEP;
    return tp;
}

// the deprojection of a depth call into its records: rule C7 for registered images, rule C12 for a mapped call
void launch_depth_job(hipStream_t s, const DepthJob* dj, int F, float4* out) {
    if (dj->ccam)
        launch_texture_map(s, dj->depth, dj->color, dj->cam->width, dj->cam->height, F, texture_params(dj->cam, dj->ccam), out);
    else
        launch_deproject(s, dj->depth, dj->color, dj->cam->width, dj->cam->height, F, dj->cam->fx, dj->cam->fy, dj->cam->cx, dj->cam->cy,
                         dj->cam->depth_scale, out);
}

// ---- depth-image input (k_depth.hip) ---------------------------------------------------------------------------------------
// every check of the header's list, before anything is copied or launched
int check_depth(cd_context* c, const cd_depth_camera* cam, const void* depth, const void* color, int n_frames) {
    if (!cam) return fail(c, CD_ERR_INVALID_ARG, "depth camera is NULL");
    if (!depth) return fail(c, CD_ERR_INVALID_ARG, "depth image is NULL");
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (cam->color != CD_COLOR_NONE && cam->color != CD_COLOR_RGB8) return fail(c, CD_ERR_INVALID_ARG, "unknown colour mode");
    if (cam->color == CD_COLOR_RGB8 && !color) return fail(c, CD_ERR_INVALID_ARG, "colour requested with a NULL colour image");
    for (float v : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(v) && v > 0.f)) return fail(c, CD_ERR_INVALID_ARG, "fx, fy and depth_scale must be finite and > 0");
    return CD_OK;
}

static_assert(sizeof(cd_color_camera) == 80 && offsetof(cd_color_camera, no_texture) == 72, "cd_color_camera has no padding holes");
// what a mapped call (rule C12) needs besides check_depth: nullptr = fine, else what is wrong (shared with the host-only
// cd_texture_project)
static const char* color_camera_error(const cd_color_camera* cc) {
    if (!cc) return "colour camera is NULL";
    if (cc->width <= 0 || cc->height <= 0) return "the colour image's width * height must be in 1 .. the context's max_points";
    for (float v : {cc->fx, cc->fy})
        if (!(std::isfinite(v) && v > 0.f)) return "the colour camera's fx and fy must be finite and > 0";
    for (float v : {cc->cx, cc->cy})
        if (!std::isfinite(v)) return "the colour camera's cx or cy is not finite";
    for (float v : cc->R) if (!std::isfinite(v)) return "R holds a non-finite value";
    for (float v : cc->t) if (!std::isfinite(v)) return "t holds a non-finite value";
    if (cc->no_texture != CD_NOTEX_DROP && cc->no_texture != CD_NOTEX_KEEP) return "unknown no_texture mode";
    return nullptr;
}

// every check of the header's list for a mapped call, before anything is copied or launched
int check_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* cc, const void* depth, const void* color, int n_frames) {
    int st = check_depth(c, cam, depth, color, n_frames);
    if (st) return st;
    if (cam->color != CD_COLOR_RGB8) return fail(c, CD_ERR_INVALID_ARG, "a mapped call needs CD_COLOR_RGB8");
    if (const char* msg = color_camera_error(cc)) return fail(c, CD_ERR_INVALID_ARG, msg);
    if ((long long)cc->width * cc->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "the colour image's width * height must be in 1 .. the context's max_points");
    return CD_OK;
}

// host images -> the context's depth / colour buffers (one copy each, on the context's stream); ccam: the colour images have
// their own size
int upload_depth(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, int n_frames, DepthJob* dj,
                 const cd_color_camera* ccam) {
    const size_t px = (size_t)cam->width * cam->height * n_frames;
    const size_t cpx = ccam ? (size_t)ccam->width * ccam->height * n_frames : px;
    GROW(c, d_depth, (size_t)c->N * c->F);
    HIPCHK(c, hipMemcpyAsync(c->d_depth, depth, px * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    dj->cam = cam;
    dj->depth = c->d_depth;
    dj->color = nullptr;
    if (cam->color == CD_COLOR_RGB8) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, color, cpx * 3, hipMemcpyHostToDevice, c->stream));
        dj->color = c->d_color;
    }
    dj->ccam = ccam;
    return CD_OK;
}
}  // namespace cd

namespace {
int cd_depth_to_cloud_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, void* out_records,
                                  size_t stride, int rgb_offset, int capacity, int* out_n, const cd_color_camera* ccam = nullptr,
                                  bool mapped = false) {
    if (!out_n || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3) ||
        (rgb_offset >= 0 && (rgb_offset < 12 || (rgb_offset & 3) || (size_t)rgb_offset + 4 > stride)))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    int st = mapped ? check_mapped(c, cam, ccam, depth, color, 1) : check_depth(c, cam, depth, color, 1);
    if (st) return st;
    *out_n = 0;
    invalidate_last(c);
    const int P = cam->width * cam->height;
    if (P > capacity) { *out_n = P; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    // one buffer: the canonical records, then (256-byte aligned) the caller's layout that goes back
    const size_t rec_bytes = (size_t)P * sizeof(float4);
    st = ensure_input(c, ((rec_bytes + 255) & ~(size_t)255) + (size_t)P * stride);
    if (st) return st;
    DepthJob dj;
    st = upload_depth(c, cam, depth, color, 1, &dj, ccam);
    if (st) return st;
    LAUNCH(c, launch_depth_job(c->stream, &dj, 1, reinterpret_cast<float4*>(c->d_in.get())));
    st = download_records(c, reinterpret_cast<const float4*>(c->d_in.get()), P, stride, rgb_offset, 0u, out_records, rec_bytes);
    if (st) return st;
    *out_n = P;
    return CD_OK;
}

// ---- colour gate as a call of its own (rule C10) ------------------------------------------------------------------------------
int cd_color_bbox_batch_impl(cd_context* c, const uint8_t* rgb8, int width, int height, int n_frames, const cd_color_gate_params* g,
                                    cd_color_bbox* out, bool on_device) {
    if (!rgb8 || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (width <= 0 || height <= 0 || (long long)width * height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    cd_color_gate_params def;
    cd_default_color_gate_params(&def);
    if (!g) g = &def;
    int st = check_color_params(c, g);
    if (st) return st;
    invalidate_last(c);
    const uint8_t* d_rgb = rgb8;
    if (!on_device) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, rgb8, (size_t)width * height * n_frames * 3, hipMemcpyHostToDevice, c->stream));
        d_rgb = c->d_color;
    }
    st = stage_color(c, d_rgb, width, height, n_frames, g);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_crec, sizeof(cd_color_bbox) * (size_t)n_frames);
    return color_status(c, n_frames);
}

// ---- the boxes of the last fused call, as cd_draw_last_results and cd_verify_last_results take them ---------------------------
// LAST_B slots per frame, slot k of frame f = cluster k of its record; n_boxes[f] = min(clusters, LAST_B).  A slot that is not
// selected (all: every cluster; otherwise the accepted ones) keeps a NaN pose and slot -1.  verb: for the error texts.
constexpr int LAST_B = CD_MAX_CLUSTERS_PER_FRAME;
struct LastBoxes {
    std::vector<double> poses;      // [F][LAST_B][16]
    std::vector<int32_t> n_boxes;   // [F]
    std::vector<int> slot;          // [F][LAST_B]: the template slot of a selected box
};

int last_frames(cd_context* c, const char* verb, int* F) {
    *F = (int)c->last_first.size() - 1;
    if (*F >= 1) return CD_OK;
    std::snprintf(c->err, sizeof(c->err), "no fused call to %s: none has run, or another compute call has run since", verb);
    return CD_ERR_INVALID_ARG;
}

int last_boxes(cd_context* c, int F, bool all, const char* verb, LastBoxes* lb) {
    lb->poses.assign((size_t)F * LAST_B * 16, std::numeric_limits<double>::quiet_NaN());
    lb->n_boxes.assign((size_t)F, 0);
    lb->slot.assign((size_t)F * LAST_B, -1);
    for (int f = 0; f < F; ++f) {
        const int lo = c->last_first[(size_t)f], hi = c->last_first[(size_t)f + 1];
        if (lo < 0 || hi < lo || (size_t)hi > c->last_clusters.size()) {
            std::snprintf(c->err, sizeof(c->err), "no fused call to %s", verb);
            return CD_ERR_INVALID_ARG;
        }
        const int n = std::min(hi - lo, LAST_B);
        lb->n_boxes[(size_t)f] = n;
        for (int k = 0; k < n; ++k) {
            const cd_cluster_result& cr = c->last_clusters[(size_t)(lo + k)];
            if (!all && !cr.accepted) continue;
            const size_t i = (size_t)f * LAST_B + k;
            std::memcpy(&lb->poses[i * 16], cr.pose, sizeof(cr.pose));
            lb->slot[i] = cr.template_slot;
        }
    }
    return CD_OK;
}

// ---- overlay (rule C11, k_overlay.hip) -----------------------------------------------------------------------------------------
static_assert(sizeof(OverlayBox) == sizeof(cd_overlay_box) && offsetof(cd_overlay_box, drawn) == offsetof(OverlayBox, drawn), "the kernel's record is cd_overlay_box");
static_assert(sizeof(cd_overlay_params) == 12 * 8 + 16 * 8 + 3 * 8 + 4 + 4 + 6 * 4 && offsetof(cd_overlay_params, reserved) == 256, "cd_overlay_params has no padding holes");
constexpr int OVERLAY_MAX_BOXES = 1024;   // boxes_per_frame of a draw call

// the checks on the parameters alone (shared with the host-only cd_overlay_project): nullptr = fine, else what is wrong
const char* overlay_params_error(const cd_overlay_params* op) {
    for (double v : op->P) if (!std::isfinite(v)) return "P holds a non-finite value";
    for (double v : op->E) if (!std::isfinite(v)) return "E holds a non-finite value";
    for (double v : op->dims) if (!std::isfinite(v)) return "dims holds a non-finite value";
    if (op->thickness < 1 || op->thickness > OVERLAY_MAX_THICKNESS) return "thickness must be in 1 .. 64";
    return nullptr;
}

// rule C11 step 2: M = P E, every entry ((p0 e0 + p1 e1) + p2 e2) + p3 e3
OverlayParams overlay_kernel_params(const cd_overlay_params* op) {
    OverlayParams k;
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col)
            k.M[4 * r + col] = ((op->P[4 * r] * op->E[col] + op->P[4 * r + 1] * op->E[4 + col]) + op->P[4 * r + 2] * op->E[8 + col]) + op->P[4 * r + 3] * op->E[12 + col];
    for (int i = 0; i < 3; ++i) k.dims[i] = op->dims[i];
    return k;
}

// every check of the header's list but those on n_boxes, before anything is copied or launched
int check_overlay(cd_context* c, const void* rgb8, int width, int height, int n_frames, const cd_overlay_params* op, const void* out) {
    if (!rgb8 || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (width <= 0 || height <= 0 || (long long)width * height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (width > OVERLAY_COORD_MAX || height > OVERLAY_COORD_MAX) return fail(c, CD_ERR_INVALID_ARG, "width and height must not exceed 8192");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (const char* msg = overlay_params_error(op)) return fail(c, CD_ERR_INVALID_ARG, msg);
    return CD_OK;
}

// poses (F * B * 16 doubles) and n_boxes (F) are HOST memory; img is device memory (on_device) or host memory that is
// uploaded, drawn on and downloaded again.  Leaves the read-back state of the last fused call alone.
int stage_overlay(cd_context* c, uint8_t* img, int W, int H, int F, const double* poses, const int32_t* n_boxes, int B,
                         const cd_overlay_params* op, cd_overlay_box* out, bool on_device) {
    const size_t nb = (size_t)F * (size_t)B;
    GROW(c, d_oposes, nb * 16); GROW(c, d_obox, nb); GROW(c, h_obox, nb);
    GROW(c, d_onbox, (size_t)c->F);
    const size_t img_bytes = (size_t)W * H * F * 3;
    uint8_t* d_img = img;
    if (!on_device) {
        GROW(c, d_color, (size_t)c->N * c->F * 3);
        HIPCHK(c, hipMemcpyAsync(c->d_color, img, img_bytes, hipMemcpyHostToDevice, c->stream));
        d_img = c->d_color;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_oposes, poses, sizeof(double) * 16 * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_onbox, n_boxes, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, c->stream));
    const OverlayParams kp = overlay_kernel_params(op);
    LAUNCH(c, launch_overlay_project(c->stream, c->d_oposes, c->d_onbox, B, F, kp, c->d_obox));
    LAUNCH(c, launch_overlay_raster(c->stream, d_img, W, H, B, F, op->thickness, op->rgb, c->d_obox));
    HIPCHK(c, hipMemcpyAsync(c->h_obox, c->d_obox, sizeof(OverlayBox) * nb, hipMemcpyDeviceToHost, c->stream));
    if (!on_device) HIPCHK(c, hipMemcpyAsync(img, d_img, img_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_obox, sizeof(cd_overlay_box) * nb);
    return CD_OK;
}

int cd_draw_boxes_batch_impl(cd_context* c, uint8_t* rgb8, int width, int height, int n_frames, const double* poses,
                                    const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out, bool on_device) {
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    int st = check_overlay(c, rgb8, width, height, n_frames, op, out);
    if (st) return st;
    if (!poses || !n_boxes) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (boxes_per_frame < 1 || boxes_per_frame > OVERLAY_MAX_BOXES) return fail(c, CD_ERR_INVALID_ARG, "boxes_per_frame must be in 1 .. 1024");
    for (int f = 0; f < n_frames; ++f)
        if (n_boxes[f] < 0 || n_boxes[f] > boxes_per_frame) return fail(c, CD_ERR_INVALID_ARG, "n_boxes[f] must be in 0 .. boxes_per_frame");
    invalidate_last(c);
    return stage_overlay(c, rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, on_device);
}

int cd_draw_last_results_impl(cd_context* c, uint8_t* rgb8, int width, int height, int which, const cd_overlay_params* op,
                                     cd_overlay_box* out, bool on_device) {
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    int F = 0;
    int st = last_frames(c, "draw", &F);
    if (!st) st = check_overlay(c, rgb8, width, height, F, op, out);
    if (st) return st;
    if (which != CD_DRAW_ACCEPTED && which != CD_DRAW_ALL) return fail(c, CD_ERR_INVALID_ARG, "unknown selection of boxes");
    LastBoxes lb;   // (a slot that is not drawn carries a NaN pose, which rule C11 skips)
    st = last_boxes(c, F, which == CD_DRAW_ALL, "draw", &lb);
    if (st) return st;
    return stage_overlay(c, rgb8, width, height, F, lb.poses.data(), lb.n_boxes.data(), LAST_B, op, out, on_device);
}

// ---- pose verification (rule C14, k_verify.hip) -----------------------------------------------------------------------------------
static_assert(sizeof(VerifyRecord) == sizeof(cd_verify_box) && sizeof(cd_verify_box) == 48 && offsetof(cd_verify_box, agree_abs_um) == offsetof(VerifyRecord, agree_abs_um) &&
              offsetof(cd_verify_box, score) == 40, "the kernel's record is cd_verify_box");
static_assert(sizeof(cd_verify_params) == (3 + 3 * CD_MAX_TEMPLATES + 2) * 8 + 8 * 4 && offsetof(cd_verify_params, reserved) == sizeof(cd_verify_params) - 24, "cd_verify_params has no padding holes");
static_assert(sizeof(VerifyJob) == 152, "152 bytes per box cross the bus");

bool verify_dim_ok(double v) { return std::isfinite(v) && v >= 0.0; }
// the checks on the camera and the parameters alone (shared with the host-only entries): nullptr = fine, else what is wrong
const char* verify_camera_error(const cd_depth_camera* cam) {
    if (!cam) return "depth camera is NULL";
    if (cam->color != CD_COLOR_NONE && cam->color != CD_COLOR_RGB8) return "unknown colour mode";
    for (float v : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(v) && v > 0.f)) return "fx, fy and depth_scale must be finite and > 0";
    return nullptr;
}
const char* verify_params_error(const cd_verify_params* vp) {
    for (double v : vp->dims) if (!verify_dim_ok(v)) return "dims must be finite and >= 0";
    if (vp->use_slot_dims)
        for (int s = 0; s < CD_MAX_TEMPLATES; ++s)
            for (double v : vp->slot_dims[s]) if (!verify_dim_ok(v)) return "slot_dims must be finite and >= 0";
    if (!verify_dim_ok(vp->tolerance)) return "tolerance must be finite and >= 0";
    if (!std::isfinite(vp->min_score)) return "min_score must be finite";
    if (vp->min_agree < 0) return "min_agree must be >= 0";
    return nullptr;
}
VerifyCam verify_kernel_camera(const cd_depth_camera* cam) {
    VerifyCam k;
    k.fx = (double)cam->fx; k.fy = (double)cam->fy; k.cx = (double)cam->cx; k.cy = (double)cam->cy; k.depth_scale = (double)cam->depth_scale;
    k.width = cam->width; k.height = cam->height;
    return k;
}
// rule C14 step 5: what the host adds to the counts
void verify_finish(const cd_verify_params* vp, cd_verify_box* r) {
    const long long den = (long long)r->n_agree + (long long)r->n_through;
    r->score = den != 0 ? (double)r->n_agree / (double)den : 0.0;
    r->passed = (r->verified && r->n_agree >= vp->min_agree && r->score >= vp->min_score) ? 1 : 0;
    r->reserved = 0;
}

// every check of the header's list but those on the boxes, before anything is copied or launched
int check_verify(cd_context* c, const cd_depth_camera* cam, const void* depth, int n_frames, const cd_verify_params* vp, const void* out) {
    if (!depth || !out) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (const char* msg = verify_camera_error(cam)) return fail(c, CD_ERR_INVALID_ARG, msg);
    if (cam->width <= 0 || cam->height <= 0 || (long long)cam->width * cam->height > (long long)c->N)
        return fail(c, CD_ERR_INVALID_ARG, "width * height must be in 1 .. the context's max_points");
    if (n_frames <= 0 || n_frames > c->F) return fail(c, CD_ERR_INVALID_ARG, "n_frames must be in 1 .. the context's max_frames");
    if (const char* msg = verify_params_error(vp)) return fail(c, CD_ERR_INVALID_ARG, msg);
    return CD_OK;
}

// poses (F * B * 16 doubles), n_boxes (F) and dims (F * B * 3 doubles) are HOST memory; depth is device memory (on_device) or host
// memory that is uploaded into d_vdepth.  Reads the images only, and leaves the read-back state of the last fused call alone.
int stage_verify(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int F, const double* poses, const int32_t* n_boxes,
                        int B, const double* dims, const cd_verify_params* vp, cd_verify_box* out, bool on_device) {
    const size_t nb = (size_t)F * (size_t)B;
    GROW(c, d_vjob, nb); GROW(c, h_vjob, nb); GROW(c, d_vrec, nb); GROW(c, h_vrec, nb);
    GROW(c, d_vnbox, (size_t)c->F); GROW(c, h_vnbox, (size_t)c->F);
    const uint16_t* d_img = depth;
    if (!on_device) {
        const size_t px = (size_t)cam->width * cam->height * F;
        GROW(c, d_vdepth, px);
        HIPCHK(c, hipMemcpyAsync(c->d_vdepth, depth, px * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        d_img = c->d_vdepth;
    }
    for (int f = 0; f < F; ++f) {
        c->h_vnbox[f] = n_boxes[f];
        for (int b = 0; b < B; ++b) {
            const size_t i = (size_t)f * B + b;
            VerifyJob& j = c->h_vjob[i];
            std::memcpy(j.pose, poses + i * 16, sizeof(j.pose));
            std::memcpy(j.dims, dims + i * 3, sizeof(j.dims));
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_vjob, c->h_vjob, sizeof(VerifyJob) * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_vnbox, c->h_vnbox, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, launch_verify_boxes(c->stream, d_img, verify_kernel_camera(cam), vp->tolerance, c->d_vjob, c->d_vnbox, B, F, c->d_vrec));
    HIPCHK(c, hipMemcpyAsync(c->h_vrec, c->d_vrec, sizeof(VerifyRecord) * nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_vrec, sizeof(cd_verify_box) * nb);
    for (int f = 0; f < F; ++f)
        for (int b = 0; b < n_boxes[f]; ++b) verify_finish(vp, out + (size_t)f * B + b);
    return CD_OK;
}

int cd_verify_boxes_batch_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, const double* poses,
                                      const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp,
                                      cd_verify_box* out, bool on_device) {
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    int st = check_verify(c, cam, depth, n_frames, vp, out);
    if (st) return st;
    if (!poses || !n_boxes) return fail(c, CD_ERR_INVALID_ARG, "null pointer");
    if (boxes_per_frame < 1 || boxes_per_frame > OVERLAY_MAX_BOXES) return fail(c, CD_ERR_INVALID_ARG, "boxes_per_frame must be in 1 .. 1024");
    const int B = boxes_per_frame;
    for (int f = 0; f < n_frames; ++f)
        if (n_boxes[f] < 0 || n_boxes[f] > B) return fail(c, CD_ERR_INVALID_ARG, "n_boxes[f] must be in 0 .. boxes_per_frame");
    std::vector<double> dims((size_t)n_frames * B * 3);
    for (size_t i = 0; i < (size_t)n_frames * B; ++i)
        for (int k = 0; k < 3; ++k) dims[i * 3 + k] = vp->dims[k];
    if (box_dims)
        for (int f = 0; f < n_frames; ++f)
            for (int b = 0; b < n_boxes[f]; ++b)
                for (int k = 0; k < 3; ++k) {
                    const size_t i = ((size_t)f * B + b) * 3 + k;
                    if (!verify_dim_ok(box_dims[i])) return fail(c, CD_ERR_INVALID_ARG, "box_dims must be finite and >= 0");
                    dims[i] = box_dims[i];
                }
    invalidate_last(c);
    return stage_verify(c, cam, depth, n_frames, poses, n_boxes, B, dims.data(), vp, out, on_device);
}

int cd_verify_last_results_impl(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int which, const cd_verify_params* vp,
                                       cd_verify_box* out, bool on_device) {
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    int F = 0;
    int st = last_frames(c, "verify", &F);
    if (!st) st = check_verify(c, cam, depth, F, vp, out);
    if (st) return st;
    if (which != CD_VERIFY_ACCEPTED && which != CD_VERIFY_ALL) return fail(c, CD_ERR_INVALID_ARG, "unknown selection of boxes");
    LastBoxes lb;   // (a slot that is not selected carries a NaN pose: verified = 0, every count 0, the zero record)
    st = last_boxes(c, F, which == CD_VERIFY_ALL, "verify", &lb);
    if (st) return st;
    std::vector<double> dims((size_t)F * LAST_B * 3);
    for (size_t i = 0; i < (size_t)F * LAST_B; ++i) {
        const int s = lb.slot[i];
        std::memcpy(&dims[i * 3], vp->use_slot_dims && s >= 0 && s < CD_MAX_TEMPLATES ? vp->slot_dims[s] : vp->dims, 3 * sizeof(double));
    }
    return stage_verify(c, cam, depth, F, lb.poses.data(), lb.n_boxes.data(), LAST_B, dims.data(), vp, out, on_device);
}
}  // namespace

extern "C" {
int cd_texture_project(const cd_depth_camera* cam, const cd_color_camera* cc, int u, int v, uint16_t d, float xyz[3], int32_t pix[2],
                       int32_t* textured) {
    if (!cam || color_camera_error(cc) || u < 0 || v < 0) return CD_ERR_INVALID_ARG;
    for (float f : {cam->fx, cam->fy, cam->depth_scale})
        if (!(std::isfinite(f) && f > 0.f)) return CD_ERR_INVALID_ARG;
    float q[3];
    int32_t px[2];
    const bool tex = texture_point(texture_params(cam, cc), (uint32_t)u, (uint32_t)v, d, q, px);
    if (xyz) std::memcpy(xyz, q, sizeof(q));
    if (pix) std::memcpy(pix, px, sizeof(px));
    if (textured) *textured = tex ? 1 : 0;
    return CD_OK;
}

int cd_color_bbox_batch(cd_context* c, const uint8_t* rgb8, int width, int height, int n_frames, const cd_color_gate_params* g, cd_color_bbox* out) {
    return with_scan_retry(c, [&] { return cd_color_bbox_batch_impl(c, rgb8, width, height, n_frames, g, out, false); });
}

int cd_color_bbox_batch_device(cd_context* c, const uint8_t* d_rgb8, int width, int height, int n_frames, const cd_color_gate_params* g, cd_color_bbox* out) {
    return with_scan_retry(c, [&] { return cd_color_bbox_batch_impl(c, d_rgb8, width, height, n_frames, g, out, true); });
}

int cd_overlay_project(const double pose[16], const cd_overlay_params* op, cd_overlay_box* out) {
    if (!pose || !out) return CD_ERR_INVALID_ARG;
    cd_overlay_params def;
    cd_default_overlay_params(&def);
    if (!op) op = &def;
    if (overlay_params_error(op)) return CD_ERR_INVALID_ARG;
    const OverlayParams kp = overlay_kernel_params(op);
    std::memset(out, 0, sizeof(*out));
    int32_t uv[16];
    for (int k = 0; k < 8; ++k) {
        float cpt[3];
        overlay_corner(pose, kp.dims, k, cpt);
        if (!overlay_pixel(kp.M, cpt, &uv[2 * k], &uv[2 * k + 1])) return CD_OK;   // skipped: the zero record
    }
    std::memcpy(out->corners, uv, sizeof(uv));
    out->drawn = 1;
    return CD_OK;
}

int cd_verify_pixel(const cd_depth_camera* cam, const double pose[16], const cd_verify_params* vp, int u, int v, uint16_t d, int32_t* cls, double* z_r) {
    if (!pose || !cls || !z_r || verify_camera_error(cam)) return CD_ERR_INVALID_ARG;
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    for (double x : vp->dims) if (!verify_dim_ok(x)) return CD_ERR_INVALID_ARG;
    if (!verify_dim_ok(vp->tolerance)) return CD_ERR_INVALID_ARG;
    VerifySetup s;
    verify_setup(pose, vp->dims, &s);
    VerifyCounts acc = {0, 0, 0, 0, 0, 0ull};
    double z = 0.0;
    *cls = verify_pixel(s, verify_kernel_camera(cam), vp->tolerance, u, v, d, &z, &acc);
    *z_r = *cls == VERIFY_MISS ? 0.0 : z;
    return CD_OK;
}

int cd_verify_box_host(const cd_depth_camera* cam, const uint16_t* depth, const double pose[16], const cd_verify_params* vp, cd_verify_box* out) {
    if (!depth || !pose || !out || verify_camera_error(cam) || cam->width < 1 || cam->height < 1) return CD_ERR_INVALID_ARG;
    cd_verify_params def;
    cd_default_verify_params(&def);
    if (!vp) vp = &def;
    if (verify_params_error(vp)) return CD_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    VerifySetup s;
    verify_setup(pose, vp->dims, &s);
    if (!s.verified) return CD_OK;   // the zero record
    const VerifyCam kc = verify_kernel_camera(cam);
    VerifyCounts acc = {0, 0, 0, 0, 0, 0ull};
    for (int v = 0; v < cam->height; ++v)
        for (int u = 0; u < cam->width; ++u) {
            double z;
            verify_pixel(s, kc, vp->tolerance, u, v, depth[(size_t)v * (size_t)cam->width + (size_t)u], &z, &acc);
        }
    out->verified = 1;
    out->n_hit = acc.n_hit; out->n_agree = acc.n_agree; out->n_through = acc.n_through; out->n_occluded = acc.n_occluded; out->n_invalid = acc.n_invalid;
    out->agree_abs_um = (int64_t)acc.agree_abs_um;
    verify_finish(vp, out);
    return CD_OK;
}

int cd_verify_boxes_batch(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp, cd_verify_box* out) {
    return with_scan_retry(c, [&] { return cd_verify_boxes_batch_impl(c, cam, depth, n_frames, poses, n_boxes, boxes_per_frame, box_dims, vp, out, false); });
}
int cd_verify_boxes_batch_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const double* box_dims, const cd_verify_params* vp, cd_verify_box* out) {
    return with_scan_retry(c, [&] { return cd_verify_boxes_batch_impl(c, cam, d_depth, n_frames, poses, n_boxes, boxes_per_frame, box_dims, vp, out, true); });
}
int cd_verify_last_results(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, int which, const cd_verify_params* vp, cd_verify_box* out) {
    return with_scan_retry(c, [&] { return cd_verify_last_results_impl(c, cam, depth, which, vp, out, false); });
}
int cd_verify_last_results_device(cd_context* c, const cd_depth_camera* cam, const uint16_t* d_depth, int which, const cd_verify_params* vp, cd_verify_box* out) {
    return with_scan_retry(c, [&] { return cd_verify_last_results_impl(c, cam, d_depth, which, vp, out, true); });
}

int cd_draw_boxes_batch(cd_context* c, uint8_t* rgb8, int width, int height, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out) {
    return with_scan_retry(c, [&] { return cd_draw_boxes_batch_impl(c, rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, false); });
}
int cd_draw_boxes_batch_device(cd_context* c, uint8_t* d_rgb8, int width, int height, int n_frames, const double* poses, const int32_t* n_boxes, int boxes_per_frame, const cd_overlay_params* op, cd_overlay_box* out) {
    return with_scan_retry(c, [&] { return cd_draw_boxes_batch_impl(c, d_rgb8, width, height, n_frames, poses, n_boxes, boxes_per_frame, op, out, true); });
}
int cd_draw_last_results(cd_context* c, uint8_t* rgb8, int width, int height, int which, const cd_overlay_params* op, cd_overlay_box* out) {
    return with_scan_retry(c, [&] { return cd_draw_last_results_impl(c, rgb8, width, height, which, op, out, false); });
}
int cd_draw_last_results_device(cd_context* c, uint8_t* d_rgb8, int width, int height, int which, const cd_overlay_params* op, cd_overlay_box* out) {
    return with_scan_retry(c, [&] { return cd_draw_last_results_impl(c, d_rgb8, width, height, which, op, out, true); });
}

int cd_depth_to_cloud(cd_context* c, const cd_depth_camera* cam, const uint16_t* depth, const uint8_t* color, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    return with_scan_retry(c, [&] { return cd_depth_to_cloud_impl(c, cam, depth, color, out_records, stride, rgb_offset, capacity, out_n); });
}
int cd_depth_to_cloud_mapped(cd_context* c, const cd_depth_camera* cam, const cd_color_camera* ccam, const uint16_t* depth, const uint8_t* color, void* out_records, size_t stride, int rgb_offset, int capacity, int* out_n) {
    return with_scan_retry(c, [&] { return cd_depth_to_cloud_impl(c, cam, depth, color, out_records, stride, rgb_offset, capacity, out_n, ccam, true); });
}
}  // extern "C"
