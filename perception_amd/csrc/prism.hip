// prism.hip - the table prism (rule C20, k_prism.hip): the step of the fused batch call, the context's setting, the read-backs of
// what the step did, the step as a call of its own and the two host helpers
#include "context.hpp"

namespace {
static_assert(sizeof(PrismRecord) == sizeof(cd_prism_stats) && offsetof(PrismRecord, overflow) == offsetof(cd_prism_stats, overflow), "the kernel's record is cd_prism_stats");

bool prism_limits_ok(double height_min, double height_max) { return std::isfinite(height_min) && std::isfinite(height_max) && height_min <= height_max; }

// the buffers of one launch over F rows with maps of `pitch` ints
int grow_prism(cd_context* c, int F, int pitch) {
    GROW(c, d_pmap, (size_t)F * pitch);
    GROW(c, d_prec, (size_t)c->F);
    GROW(c, h_prec, (size_t)c->F);
    GROW(c, d_plrec, (size_t)c->F);
    GROW(c, d_phull, (size_t)c->F * 2 * PRISM_MAX_HULL);
    return CD_OK;
}
}  // namespace

namespace cd {
// The fused call's step between stage_extract / sync_fs and stage_outlier, skipped when the step is off.
// in: d_obj + fs.n_o (max_no: the largest, as the host read it), the plane index list d_plane_idx + fs.n_plane into d_vox, the
// refined planes as stage_extract read them.  out: d_obj = the kept points of every frame in their order (compacted into d_src,
// which is free until the cluster stage, and the two buffers swapped), fs.n_o on the device and in the host's mirror, d_pmap
// (rows of *map_pitch ints: a point's index in the kept cloud or -1), d_plrec, d_phull, d_prec and - by a transfer that the
// cluster stage's synchronisation covers - h_prec.  Scratch: d_src0 (free until the cluster stage; 8 of a point's 16 bytes).
// Issues one kernel and that transfer; may grow its buffers (which synchronises the stream); synchronises nothing else.
int stage_prism(cd_context* c, int F, int max_no, int* map_pitch) {
    const int pitch = (std::max(max_no, 1) + 63) & ~63;
    *map_pitch = pitch;
    if (int st = grow_prism(c, F, pitch)) return st;
    PrismArgs a;
    a.plane_pts = c->d_vox; a.plane_idx = c->d_plane_idx;
    a.model = c->tun.mirror_reads ? c->h_model : c->d_model;   // (as stage_extract read them)
    a.have = c->tun.mirror_reads ? c->h_active : c->d_have;
    a.pts = c->d_obj; a.N = c->N;
    a.fs = c->d_fs; a.mirror = c->tun.mirror_writes && c->tun.copy_kernels ? c->h_fs.get() : nullptr;
    a.hmin = c->prism_hmin; a.hmax = c->prism_hmax;
    a.scratch = reinterpret_cast<int2*>(c->d_src0.get());
    a.out = c->d_src; a.map = c->d_pmap; a.mpitch = pitch; a.kept_idx = nullptr;
    a.rec = c->d_prec; a.lrec = c->d_plrec; a.hull = c->d_phull;
    LAUNCH(c, launch_prism(c->stream, F, a));
    std::swap(c->d_obj, c->d_src);
    HIPCHK(c, xfer(c, c->h_prec, c->d_prec, sizeof(PrismRecord) * (size_t)F, hipMemcpyDeviceToHost));
    return CD_OK;
}

// With the outlier filter behind the prism (stage_outlier has run with the same max_no, so d_omap has rows of the same pitch):
// d_pmap becomes S3 index -> prism -> filter, the one map the label calls take.  Issues one kernel.
int prism_compose_map(cd_context* c, int F, int map_pitch) {
    LAUNCH(c, launch_prism_compose_map(c->stream, F, c->d_pmap, c->d_plrec, c->d_omap, map_pitch));
    return CD_OK;
}
}  // namespace cd

namespace {
// One cloud as row 0: the plane inliers to d_vox, the points to d_obj, the map to d_pmap, the kept indices to d_cand
int table_prism_impl(cd_context* c, const void* plane_xyz, size_t plane_stride, int n_plane, const float* coeff, const void* xyz, size_t stride, int n,
                     double height_min, double height_max, int32_t* out_indices, int capacity, int* out_n, cd_prism_stats* stats, int32_t* hull_uv,
                     int hull_capacity) {
    invalidate_last(c);
    if ((!xyz && n > 0) || (!plane_xyz && n_plane > 0) || !coeff || !out_n || n < 0 || n_plane < 0 || capacity < 0 || (capacity > 0 && !out_indices) ||
        stride < 12 || (stride & 3) || plane_stride < 12 || (plane_stride & 3) || hull_capacity < 0 || (hull_capacity > 0 && !hull_uv))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (!prism_limits_ok(height_min, height_max)) return fail(c, CD_ERR_INVALID_ARG, "height_min and height_max must be finite with height_min <= height_max");
    *out_n = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n > c->N || n_plane > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    const int pitch = (std::max(n, 1) + 63) & ~63;
    int st = grow_prism(c, 1, pitch);
    if (st) return st;
    if (n_plane > 0) st = upload_points(c, plane_xyz, plane_stride, n_plane, c->d_vox);
    if (!st && n > 0) st = upload_points(c, xyz, stride, n, c->d_obj);
    if (st) return st;
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    c->h_fs[0].n_o = n;
    c->h_fs[0].n_plane = n_plane;
    c->h_model[0] = make_float4(coeff[0], coeff[1], coeff[2], coeff[3]);
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    HIPCHK(c, xfer(c, c->d_model, c->h_model, sizeof(float4), hipMemcpyHostToDevice));
    PrismArgs a;
    a.plane_pts = c->d_vox; a.plane_idx = nullptr; a.model = c->d_model; a.have = nullptr;
    a.pts = c->d_obj; a.N = c->N;
    a.fs = c->d_fs; a.mirror = nullptr;
    a.hmin = height_min; a.hmax = height_max;
    a.scratch = reinterpret_cast<int2*>(c->d_src0.get());
    a.out = nullptr; a.map = c->d_pmap; a.mpitch = pitch; a.kept_idx = c->d_cand;
    a.rec = c->d_prec; a.lrec = c->d_plrec; a.hull = c->d_phull;
    LAUNCH(c, launch_prism(c->stream, 1, a));
    HIPCHK(c, copy_sync(c, c->h_prec, c->d_prec, sizeof(PrismRecord), hipMemcpyDeviceToHost));
    const PrismRecord& r = c->h_prec[0];
    if (r.n_before != n || r.n_kept < 0 || r.n_kept > n || r.hull_vertices < 0 || r.hull_vertices > PRISM_MAX_HULL)
        return fail(c, CD_ERR_DEVICE, "the prism kernel left an inconsistent record");
    if (stats) std::memcpy(stats, &r, sizeof(*stats));
    *out_n = r.n_kept;
    if (r.n_kept > capacity) return fail(c, CD_ERR_CAPACITY, "index capacity too small");
    if (r.n_kept > 0) HIPCHK(c, copy_sync(c, out_indices, c->d_cand, sizeof(int) * (size_t)r.n_kept, hipMemcpyDeviceToHost));
    if (hull_uv) {
        if (r.hull_vertices > hull_capacity) return fail(c, CD_ERR_CAPACITY, "hull capacity too small");
        if (r.hull_vertices > 0) HIPCHK(c, copy_sync(c, hull_uv, c->d_phull, sizeof(int32_t) * 2 * (size_t)r.hull_vertices, hipMemcpyDeviceToHost));
    }
    return CD_OK;
}
}  // namespace

extern "C" {
int cd_set_table_prism(cd_context* c, int enable, double height_min, double height_max) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!prism_limits_ok(height_min, height_max)) return fail(c, CD_ERR_INVALID_ARG, "height_min and height_max must be finite with height_min <= height_max");
    c->prism_on = enable ? 1 : 0;
    c->prism_hmin = height_min;
    c->prism_hmax = height_max;
    return CD_OK;
}

int cd_get_table_prism(const cd_context* c, int* enable, double* height_min, double* height_max) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (enable) *enable = c->prism_on;
    if (height_min) *height_min = c->prism_hmin;
    if (height_max) *height_max = c->prism_hmax;
    return CD_OK;
}

int cd_prism_struct_size(void) { return (int)sizeof(cd_prism_stats); }

int cd_get_prism_stats(const cd_context* c, int frame, cd_prism_stats* out) {
    if (!c || !out) return CD_ERR_INVALID_ARG;
    if (!c->last_prism_ok || !c->last_clouds || frame < 0 || (size_t)frame >= c->last_prism.size() || (size_t)frame + 1 >= c->last_first.size())
        return CD_ERR_INVALID_ARG;   // (const: no message; the call ran without the step, has been invalidated, or had no such frame)
    std::memcpy(out, &c->last_prism[(size_t)frame], sizeof(*out));
    return CD_OK;
}

int cd_get_prism_hull(cd_context* c, int frame, int32_t* uv, int capacity, int* n) {
    if (!c) return CD_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (!n || capacity < 0 || (capacity > 0 && !uv)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *n = 0;
    if (!c->last_prism_ok || !c->last_clouds || frame < 0 || (size_t)frame >= c->last_prism.size() || (size_t)frame + 1 >= c->last_first.size())
        return fail(c, CD_ERR_INVALID_ARG, "not a frame of the last fused call of this context, or that call ran without the table prism");
    const int m = std::min(std::max(c->last_prism[(size_t)frame].hull_vertices, 0), PRISM_MAX_HULL);
    *n = m;
    if (m > capacity) return fail(c, CD_ERR_CAPACITY, "hull capacity too small");
    if (m > 0) HIPCHK(c, copy_sync(c, uv, c->d_phull + (size_t)frame * 2 * PRISM_MAX_HULL, sizeof(int32_t) * 2 * (size_t)m, hipMemcpyDeviceToHost));
    return CD_OK;
}

int cd_table_prism(cd_context* c, const void* plane_xyz, size_t plane_stride, int n_plane, const float coeff[4], const void* xyz, size_t stride_bytes, int n,
                   double height_min, double height_max, int32_t* out_indices, int capacity, int* out_n, cd_prism_stats* stats, int32_t* hull_uv,
                   int hull_capacity) {
    return with_scan_retry(c, [&] {
        return table_prism_impl(c, plane_xyz, plane_stride, n_plane, coeff, xyz, stride_bytes, n, height_min, height_max, out_indices, capacity, out_n, stats,
                                hull_uv, hull_capacity);
    });
}

int cd_prism_project(const float coeff[4], const float xyz[3], double* height, int32_t uv[2], int32_t axes[2]) {
    if (!coeff || !xyz) return CD_ERR_INVALID_ARG;
    const PrismPlane P = prism_plane(coeff[0], coeff[1], coeff[2], coeff[3]);
    double h;
    int32_t u, v;
    prism_project(P, xyz[0], xyz[1], xyz[2], &h, &u, &v);
    if (height) *height = h;
    if (uv) { uv[0] = u; uv[1] = v; }
    if (axes) { axes[0] = P.k1; axes[1] = P.k2; }
    return CD_OK;
}

int cd_prism_hull_host(const int32_t* uv, int n, int32_t* hull, int capacity, int* n_hull) {
    if (n < 0 || (n > 0 && !uv) || capacity < 0 || (capacity > 0 && !hull) || !n_hull) return CD_ERR_INVALID_ARG;
    *n_hull = prism_hull_host(uv, n, hull, capacity);
    return *n_hull > capacity ? CD_ERR_CAPACITY : CD_OK;
}
}  // extern "C"
