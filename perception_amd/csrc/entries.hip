// entries.hip - the per-stage entry points: crop + voxel grid, plane, surface normals, bbox filter, extract, passthrough,
// cluster, ICP, ground plane and shape frames.  Each `X_impl` runs under with_scan_retry (context.hpp).
#include "context.hpp"
#include "host_math.hpp"
#include "icp_solve_row.hpp"

namespace {
int cd_crop_voxel_impl(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float* out_xyz,
                  uint32_t* out_rgb, int capacity, int* out_n_cropped, int* out_n_voxels) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!points || !out_xyz || n < 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (out_n_cropped) *out_n_cropped = 0;
    if (out_n_voxels) *out_n_voxels = 0;
    if (n == 0) return CD_OK;
    st = ensure_input(c, (size_t)n * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    st = stage_crop_voxel(c, c->d_in, stride, n, 1, p, nullptr);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const FrameState& s = c->h_fs[0];
    if (out_n_cropped) *out_n_cropped = s.n_cropped;
    if (s.status != CD_OK) return fail(c, s.status, "voxel grid: leaf size too small for the input extent");
    if (s.n_v > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    std::vector<float4> tmp((size_t)std::max(s.n_v, 1));
    HIPCHK(c, copy_sync(c, tmp.data(), c->d_vox, sizeof(float4) * s.n_v, hipMemcpyDeviceToHost));
    for (int i = 0; i < s.n_v; ++i) {
        out_xyz[3 * i] = tmp[i].x; out_xyz[3 * i + 1] = tmp[i].y; out_xyz[3 * i + 2] = tmp[i].z;
        if (out_rgb) std::memcpy(&out_rgb[i], &tmp[i].w, 4);
    }
    if (out_n_voxels) *out_n_voxels = s.n_v;
    return CD_OK;
}

// helper: load a caller cloud as the (single-frame) voxel cloud / object cloud
int load_as(cd_context* c, const void* xyz, size_t stride, int n, float4* dst, int32_t FrameState::*count) {
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    int st = upload_points(c, xyz, stride, n, dst);
    if (st) return st;
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    c->h_fs[0].*count = n;
    // origin for the cluster hash: min of the cloud
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    const char* b = (const char*)xyz;
    for (int i = 0; i < n; ++i) {
        float v[3];
        std::memcpy(v, b + (size_t)i * stride, 12);
        for (int a = 0; a < 3; ++a) if (v[a] < mn[a]) mn[a] = v[a];
    }
    for (int a = 0; a < 3; ++a) c->h_fs[0].origin[a] = n > 0 ? mn[a] : 0.f;
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    return CD_OK;
}

int cd_segment_plane_impl(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, float coeff[4],
                     int32_t* inliers, int capacity, int* out_n_inliers, int* out_iterations) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!xyz || !coeff || !inliers || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (out_n_inliers) *out_n_inliers = 0;
    if (out_iterations) *out_iterations = 0;
    st = load_as(c, xyz, stride, n, c->d_vox, &FrameState::n_v);
    if (st) return st;
    std::vector<int> iters;
    st = stage_plane(c, 1, p, iters, nullptr);
    if (st) return st;
    if (out_iterations) *out_iterations = iters[0];
    if (c->plane_gave_up[0]) return CD_ERR_CAPACITY;   // (cd_last_error names the limit: stage_plane)
    if (!c->h_have[0]) return CD_ERR_NO_MODEL;
    cd_params q = *p;
    q.extract_negative = 1;
    q.crop2_enable = 0;
    st = stage_extract(c, 1, &q);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int ni = c->h_fs[0].n_plane;
    if (ni > capacity) return fail(c, CD_ERR_CAPACITY, "inlier capacity too small");
    if (ni > 0) HIPCHK(c, copy_sync(c, inliers, c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
    coeff[0] = c->h_model[0].x; coeff[1] = c->h_model[0].y; coeff[2] = c->h_model[0].z; coeff[3] = c->h_model[0].w;
    if (out_n_inliers) *out_n_inliers = ni;
    return CD_OK;
}

// surface_normal_estimation.cpp:167-234.  The three constrained fits run on the device (cd_segment_plane's
// stages); the bookkeeping between them (ExtractIndices, pcl::compute3DCentroid - a sequential float32 sum -,
// the size sort, the handedness flip and the pose assembly) is the callback's own host code.
int cd_surface_frame_impl(cd_context* c, const void* xyz, size_t stride, int n, const float table_normal[3], int invert,
                     const cd_params* p, cd_surface_frame_result* out) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if ((!xyz && n > 0) || !table_normal || !out || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    std::memset(out, 0, sizeof(*out));
    struct P3 { float x, y, z; };
    std::vector<P3> cloud((size_t)n);
    for (int i = 0; i < n; ++i) std::memcpy(&cloud[(size_t)i], (const char*)xyz + (size_t)i * stride, 12);
    float normals[3][4], mids[3][4];
    int counts[3];
    for (int i = 0; i < 3; ++i) {   // sne.cpp:183-197
        cd_params q = *p;
        q.plane_model = i == 0 ? CD_PLANE_PERPENDICULAR : CD_PLANE_PARALLEL;
        for (int a = 0; a < 3; ++a) q.plane_axis[a] = table_normal[a];
        q.plane_eps_angle = 0.1;                       // sne.cpp:123
        q.plane_optimize = 1;                          // sne.cpp:118
        q.plane_max_iterations = 1000;                 // sne.cpp:125
        q.extract_negative = 1;
        q.crop2_enable = 0;
        q.bbox_enable = 0;
        const int m = (int)cloud.size();
        if (m > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
        st = load_as(c, cloud.data(), sizeof(P3), m, c->d_vox, &FrameState::n_v);
        if (st) return st;
        std::vector<int> iters;
        st = stage_plane(c, 1, &q, iters, nullptr);
        if (st) return st;
        out->iterations[i] = iters[0];
        if (!c->h_have[0]) return CD_ERR_NO_MODEL;
        st = stage_extract(c, 1, &q);
        if (st) return st;
        st = sync_fs(c, 1);
        if (st) return st;
        const int ni = c->h_fs[0].n_plane;
        std::vector<int> inl((size_t)std::max(ni, 1));
        if (ni > 0) HIPCHK(c, copy_sync(c, inl.data(), c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
        // getNormal(): plane_pc = ExtractIndices(negative = !invert), leftover = ExtractIndices(negative = invert)
        std::vector<char> is_inl((size_t)std::max(m, 1), 0);
        for (int k = 0; k < ni; ++k) is_inl[(size_t)inl[(size_t)k]] = 1;
        std::vector<P3> plane_pc, leftover;
        for (int k = 0; k < m; ++k) {
            const bool in = is_inl[(size_t)k] != 0;
            if (in == (invert != 0)) plane_pc.push_back(cloud[(size_t)k]); else leftover.push_back(cloud[(size_t)k]);
        }
        // pcl::compute3DCentroid: sequential float32 sums, then one division per component
        float cs[3] = {0.f, 0.f, 0.f};
        for (const P3& q3 : plane_pc) { cs[0] += q3.x; cs[1] += q3.y; cs[2] += q3.z; }
        const float cnt = (float)plane_pc.size();
        for (int a = 0; a < 3; ++a) mids[i][a] = cs[a] / cnt;
        mids[i][3] = 0.f;
        normals[i][0] = c->h_model[0].x; normals[i][1] = c->h_model[0].y; normals[i][2] = c->h_model[0].z; normals[i][3] = c->h_model[0].w;
        counts[i] = (int)plane_pc.size();
        cloud.swap(leftover);
    }
    surface_record(counts, normals, mids, out);
    return CD_OK;
}

// cd_surface_frame over a batch: the records go up as they are, k_surface_load unpacks them on the device (no host loop over
// points) and stage_surface runs the three fits of every frame together
int cd_surface_batch_impl(cd_context* c, const void* xyz, size_t stride, int P, const int32_t* n_points, int F,
                                 const float* table_normals, int invert, const cd_params* p, cd_surface_frame_result* out, int32_t* status) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!n_points || !table_normals || !out || !status || F <= 0 || P < 0 || stride < 12 || (stride & 3)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    int max_n = 0;
    for (int f = 0; f < F; ++f) {
        if (n_points[f] < 0 || n_points[f] > P) return fail(c, CD_ERR_INVALID_ARG, "n_points[f] outside [0, points_per_frame]");
        max_n = std::max(max_n, (int)n_points[f]);
    }
    if (max_n > 0 && !xyz) return fail(c, CD_ERR_INVALID_ARG, "xyz is NULL");
    if (F > c->F || max_n > c->N) return fail(c, CD_ERR_CAPACITY, "batch larger than the context capacity");
    const int pitch = std::max(max_n, 1);
    st = ensure_surface(c, (size_t)pitch);
    if (st) return st;
    std::vector<int> count(n_points, n_points + F);
    for (int f = 0; f < F; ++f) {
        std::memset(&c->h_sfs[f], 0, sizeof(FrameState));
        c->h_sfs[f].n_v = count[(size_t)f];
    }
    HIPCHK(c, xfer(c, c->d_sfs, c->h_sfs, sizeof(FrameState) * F, hipMemcpyHostToDevice));
    if (max_n > 0) {
        const size_t bytes = ((size_t)(F - 1) * P + (size_t)n_points[F - 1]) * stride;
        st = ensure_input(c, std::max<size_t>(bytes, 16));
        if (st) return st;
        if (bytes > 0) HIPCHK(c, hipMemcpyAsync(c->d_in, xyz, bytes, hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, launch_surface_load(c->stream, c->d_in, stride, stride * (size_t)P, (const int*)((char*)c->d_sfs.get() + offsetof(FrameState, n_v)),
                                      FS_PITCH, pitch, max_n, F, c->d_spts[0]));
    }
    const std::vector<char> run((size_t)F, 1);
    return stage_surface(c, F, pitch, count, table_normals, run, invert, p, out, status);
}

int cd_bbox_filter_impl(cd_context* c, const void* xyz, size_t stride, int n, const double P[12], const int32_t rect[4],
                   int32_t* out_indices, int capacity, int* out_n) {
    invalidate_last(c);
    if ((!xyz && n > 0) || !P || !rect || !out_indices || !out_n || n < 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n == 0) return CD_OK;
    int st = load_as(c, xyz, stride, n, c->d_vox, &FrameState::n_v);
    if (st) return st;
    cd_params q;
    cd_default_params(&q);
    for (int i = 0; i < 12; ++i) q.bbox_P[i] = P[i];
    for (int i = 0; i < 4; ++i) q.bbox_rect[i] = rect[i];
    HIPCHK(c, hipMemsetAsync(c->d_have, 0, sizeof(int), c->stream));
    c->h_active[0] = 0;   // (no plane: with mirror reads the kernels look here; no kernel of this context is in flight)
    st = stage_extract(c, 1, &q, 2);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int ni = c->h_fs[0].n_plane;
    if (ni > capacity) return fail(c, CD_ERR_CAPACITY, "index capacity too small");
    if (ni > 0) HIPCHK(c, copy_sync(c, out_indices, c->d_plane_idx, sizeof(int) * ni, hipMemcpyDeviceToHost));
    *out_n = ni;
    return CD_OK;
}

int cd_extract_impl(cd_context* c, const void* points, size_t stride, int n, const int32_t* indices, int n_indices, int negative,
               void* out_points, int capacity, int* out_n) {
    invalidate_last(c);
    if ((!points && n > 0) || (!indices && n_indices > 0) || !out_n || n < 0 || n_indices < 0 || capacity < 0 || stride < 4 || (stride & 3) ||
        (!out_points && capacity > 0))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n > c->N || (!negative && n_indices > c->N)) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_OK;
    const int words = (int)(stride / 4);
    // staging buffer: the input records, then room for the records that are kept
    const size_t in_bytes = ((size_t)n * stride + 255) & ~(size_t)255;
    int st = ensure_input(c, in_bytes + (size_t)(negative ? n : n_indices) * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    // index list -> d_label (upload), kept indices -> d_plane_idx
    const int mi = std::min(n_indices, c->N);
    if (mi > 0) HIPCHK(c, hipMemcpyAsync(c->d_label, indices, sizeof(int) * (size_t)mi, hipMemcpyHostToDevice, c->stream));
    int kept = 0;
    const int* d_keep = c->d_label;
    if (negative) {
        if (n_indices > c->N) return fail(c, CD_ERR_CAPACITY, "index list longer than the context capacity");
        std::memset(&c->h_fs[0], 0, sizeof(FrameState));
        HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemsetAsync(c->d_rank, 0, sizeof(int) * (size_t)n, c->stream));            // marks
        HIPCHK(c, hipMemsetAsync(c->d_tileA, 0, sizeof(int) * (size_t)c->T, c->stream));          // chained-scan state
        HIPCHK(c, hipMemsetAsync(c->d_ticket, 0, sizeof(int), c->stream));
        LAUNCH(c, launch_mark_indices(c->stream, c->d_label, mi, n, c->d_rank));
        LAUNCH(c, launch_select_unmarked(c->stream, c->d_rank, n, c->d_tileA, c->d_fs, c->d_plane_idx, c->d_ticket));
        st = sync_fs(c, 1);
        if (st) return st;
        kept = c->h_fs[0].n_plane;
        d_keep = c->d_plane_idx;
    } else {
        for (int i = 0; i < n_indices; ++i)
            if (indices[i] < 0 || indices[i] >= n) return fail(c, CD_ERR_INVALID_ARG, "index out of range");
        kept = n_indices;
    }
    if (kept > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    if (kept > 0) {
        char* d_out = (char*)c->d_in + in_bytes;
        LAUNCH(c, launch_gather_records(c->stream, c->d_in, words, d_keep, kept, d_out));
        HIPCHK(c, copy_sync(c, out_points, d_out, (size_t)kept * stride, hipMemcpyDeviceToHost));
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the uploads read caller memory
    }
    *out_n = kept;
    return CD_OK;
}

int cd_passthrough_impl(cd_context* c, const void* points, size_t stride, int n, int field, double lo, double hi, int negative,
                               void* out_points, int capacity, int* out_n) {
    invalidate_last(c);
    if ((!points && n > 0) || !out_n || n < 0 || capacity < 0 || stride < 12 || (stride & 3) || (!out_points && capacity > 0) || field < -1 || field > 2)
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_OK;
    const int words = (int)(stride / 4);
    const size_t in_bytes = ((size_t)n * stride + 255) & ~(size_t)255;   // staging: the input records, then the records that are kept
    int st = ensure_input(c, in_bytes + (size_t)n * stride);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_tileA, 0, sizeof(int) * (size_t)c->T, c->stream));          // chained-scan state
    HIPCHK(c, hipMemsetAsync(c->d_ticket, 0, sizeof(int), c->stream));
    LAUNCH(c, launch_passthrough_mark(c->stream, c->d_in, stride, n, field < 0 ? -1 : 4 * field, lo, hi, negative ? 1 : 0, c->d_rank));
    LAUNCH(c, launch_select_unmarked(c->stream, c->d_rank, n, c->d_tileA, c->d_fs, c->d_plane_idx, c->d_ticket));
    st = sync_fs(c, 1);
    if (st) return st;
    const int kept = c->h_fs[0].n_plane;
    if (kept > capacity) return fail(c, CD_ERR_CAPACITY, "output capacity too small");
    if (kept > 0) {
        char* d_out = (char*)c->d_in + in_bytes;
        LAUNCH(c, launch_gather_records(c->stream, c->d_in, words, c->d_plane_idx, kept, d_out));
        HIPCHK(c, copy_sync(c, out_points, d_out, (size_t)kept * stride, hipMemcpyDeviceToHost));
    }
    *out_n = kept;
    return CD_OK;
}

int cd_cluster_impl(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, int32_t* labels,
               int32_t* sizes, int sizes_capacity, int* out_k) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!xyz || !labels || n < 0 || stride < 12 || (sizes_capacity > 0 && !sizes)) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (out_k) *out_k = 0;
    if (n == 0) return CD_OK;
    st = load_as(c, xyz, stride, n, c->d_obj, &FrameState::n_o);
    if (st) return st;
    st = stage_cluster_sync(c, 1, p, n);
    if (st) return st;
    HIPCHK(c, copy_sync(c, labels, c->d_label, sizeof(int) * n, hipMemcpyDeviceToHost));
    const int K = c->h_fs[0].n_k;
    const int ks = std::min(K, sizes_capacity);
    if (ks > 0) HIPCHK(c, copy_sync(c, sizes, c->d_sizes, sizeof(int) * ks, hipMemcpyDeviceToHost));
    if (out_k) *out_k = K;
    return CD_OK;
}

int cd_icp_impl(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const cd_params* p,
           cd_cluster_result* out, float* aligned) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if (!src_xyz || !out || n < 0 || stride < 12 || slot < 0 || slot >= CD_MAX_TEMPLATES) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (p->icp_use_guess == CD_GUESS_SURFACE) return fail(c, CD_ERR_INVALID_ARG, "icp_use_guess = CD_GUESS_SURFACE needs a frame to fit: fused calls only");
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (c->tpl_m[slot] <= 0) return fail(c, CD_ERR_NO_TEMPLATE, "template slot is empty");
    st = check_icp_modes(c, slot);   // rule C17: lattice templates only; rule C19: not together with rule C17
    if (st) return st;
    st = upload_points(c, src_xyz, stride, n, c->d_src0);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_src, c->d_src0, sizeof(float4) * (size_t)std::max(n, 1), hipMemcpyDeviceToDevice, c->stream));
    const int off0 = 0;
    set_icp_clusters(c, 0, 1, 0, &n, &off0, 0, slot);
    st = stage_icp_levels(c, 1, p, nullptr);
    if (st) return st;
    fill_cluster_result(c, 0, p, out);
    out->template_slot = slot;
    if (aligned && n > 0) {
        std::vector<float4> tmp((size_t)n);
        HIPCHK(c, copy_sync(c, tmp.data(), c->d_src, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { aligned[3 * i] = tmp[i].x; aligned[3 * i + 1] = tmp[i].y; aligned[3 * i + 2] = tmp[i].z; }
    }
    // the pair's record for cd_get_cluster_{coarse,plane,reject}_stats (frame 0, index 0), before the return of a stop below; a
    // source of fewer than three points never reached the plane or reject kernels: an all-zero record
    if (c->coarse_stride != 0) c->last_coarse.publish_single(c->h_cstat[0]);   // rule C18
    if (c->plane_weight != 0.0) {   // rule C17
        if (n >= 3) c->last_plane.publish_single(c->h_pstat[0]);
        else c->last_plane.publish_single(cd_icp_plane_stats());
        if (c->last_plane[0].stopped_singular) return fail(c, CD_ERR_FEW_CORRESPONDENCES, "plane-weighted ICP stopped: the step's system is singular");
    }
    if (c->reject_factor != 0.0) {   // rule C19
        if (n >= 3) c->last_reject.publish_single(c->h_rstat[0]);
        else c->last_reject.publish_single(cd_icp_reject_stats());
    }
    if (c->recip_on) {   // rule C22
        if (n >= 3) c->last_recip.publish_single(c->h_qstat[0]);
        else c->last_recip.publish_single(cd_icp_recip_stats());
    }
    // rules C8, C19 and C22: an ICP that stopped for fewer than three kept correspondences (only a bounded or rejecting one can:
    // every other ends converged)
    if (c->h_st[0].status == CD_OK && (c->icp_bounded || c->reject_factor != 0.0 || c->recip_on) && !c->h_st[0].converged) return CD_ERR_FEW_CORRESPONDENCES;
    return c->h_st[0].status;
}

int cd_ground_plane_impl(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float coeff[4], void* out_records,
                    int capacity, int* out_n, int* out_n_inliers) {
    invalidate_last(c);
    int st = check_params(c, p);
    if (st) return st;
    if ((!points && n > 0) || !coeff || !out_n || n < 0 || capacity < 0 || (capacity > 0 && !out_records) || stride < 12 || (stride & 3))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    *out_n = 0;
    if (out_n_inliers) *out_n_inliers = 0;
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_ERR_NO_MODEL;
    // one buffer: the input blob, then (256-byte aligned) room for the records that go back
    const size_t in_bytes = (size_t)n * stride;
    st = ensure_input(c, ((in_bytes + 255) & ~(size_t)255) + in_bytes);
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->d_in, points, in_bytes, hipMemcpyHostToDevice, c->stream));   // the ONE upload
    st = stage_crop_voxel(c, c->d_in, stride, n, 1, p, nullptr);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    if (c->h_fs[0].status != CD_OK) return fail(c, c->h_fs[0].status, "voxel grid: leaf size too small for the input extent");
    std::vector<int> iters;
    st = stage_plane(c, 1, p, iters, nullptr);
    if (st) return st;
    st = stage_extract(c, 1, p);
    if (st) return st;
    st = sync_fs(c, 1);
    if (st) return st;
    const int no = c->h_fs[0].n_o;
    if (out_n_inliers) *out_n_inliers = c->h_fs[0].n_plane;
    if (no > capacity) { *out_n = no; return fail(c, CD_ERR_CAPACITY, "output capacity too small"); }
    const int rgb_off = (p->rgb_offset >= 12 && !(p->rgb_offset & 3) && (size_t)p->rgb_offset + 4 <= stride) ? p->rgb_offset : -1;
    st = download_records(c, c->d_obj, no, stride, rgb_off, 0u, out_records, in_bytes);               // the ONE download
    if (st) return st;
    *out_n = no;
    if (c->plane_gave_up[0]) return CD_ERR_CAPACITY;   // (cd_last_error names the limit: stage_plane)
    if (!c->h_have[0]) return CD_ERR_NO_MODEL;
    coeff[0] = c->h_model[0].x; coeff[1] = c->h_model[0].y; coeff[2] = c->h_model[0].z; coeff[3] = c->h_model[0].w;
    return CD_OK;
}

int cd_shape_frames_impl(cd_context* c, const void* xyz, size_t stride, const int32_t* offsets, int n_sets, cd_shape_frame* out) {
    if (!offsets || !out || n_sets <= 0 || stride < 12 || offsets[0] < 0) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    for (int i = 0; i < n_sets; ++i) if (offsets[i + 1] < offsets[i]) return fail(c, CD_ERR_INVALID_ARG, "offsets must ascend");
    const int base = offsets[0], total = offsets[n_sets] - base;
    if (total > 0 && !xyz) return fail(c, CD_ERR_INVALID_ARG, "null points");
    invalidate_last(c);
    GROW(c, d_shpts, (size_t)std::max(total, 1));
    GROW(c, d_shcl, (size_t)n_sets);
    GROW(c, d_shape, (size_t)n_sets);
    std::vector<IcpCluster> sets((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) sets[(size_t)i] = IcpCluster{offsets[i] - base, offsets[i + 1] - offsets[i], 0, i, 0, 0, 0, 0};
    int st = upload_points(c, (const char*)xyz + (size_t)base * stride, stride, total, c->d_shpts);
    if (st) return st;
    HIPCHK(c, copy_sync(c, c->d_shcl, sets.data(), sizeof(IcpCluster) * (size_t)n_sets, hipMemcpyHostToDevice));
    LAUNCH(c, launch_shape_frames(c->stream, n_sets, c->d_shcl, c->d_shpts, c->d_shape, nullptr, nullptr, nullptr));
    HIPCHK(c, copy_sync(c, out, c->d_shape, sizeof(ShapeFrame) * (size_t)n_sets, hipMemcpyDeviceToHost));
    return CD_OK;
}
}  // namespace

extern "C" {
// ---- rule C13: principal frames and the per-cluster guess ---------------------------------------------------
int cd_shape_frame_struct_size(void) { return (int)sizeof(cd_shape_frame); }

int cd_shape_frame_host(const void* xyz, size_t stride, int n, cd_shape_frame* out) {
    if (!out || n < 0 || (n > 0 && !xyz) || stride < 12) return CD_ERR_INVALID_ARG;
    ShapeFrame rec;
    shape_frame_host(xyz, stride, n, &rec);
    std::memcpy(out, &rec, sizeof(rec));
    return rec.status;
}

int cd_shape_guess(const cd_shape_frame* cluster, const cd_shape_frame* template_, float guess[16], int32_t* flip) {
    if (!cluster || !template_ || !guess) return CD_ERR_INVALID_ARG;
    ShapeFrame cr, tr;
    std::memcpy(&cr, cluster, sizeof(cr));
    std::memcpy(&tr, template_, sizeof(tr));
    const int k = shape_guess(cr, tr, guess);
    if (flip) *flip = k;
    return CD_OK;
}

int cd_template_shape_frame(const cd_context* c, int slot, cd_shape_frame* out) {
    if (!c || !out || slot < 0 || slot >= CD_MAX_TEMPLATES) return CD_ERR_INVALID_ARG;
    if (c->tpl_m[slot] <= 0) return CD_ERR_NO_TEMPLATE;
    std::memcpy(out, &c->tpl_frame[slot], sizeof(*out));
    return CD_OK;
}

int cd_get_cluster_shape_frames(const cd_context* c, int frame, int first, int capacity, cd_shape_frame* out) {
    return c ? c->last_shapes.read(frame, first, capacity, out) : CD_ERR_INVALID_ARG;   // (valid after a fused call in CD_GUESS_CLUSTER mode)
}

int cd_crop_voxel(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float* out_xyz, uint32_t* out_rgb, int capacity, int* out_n_cropped, int* out_n_voxels) {
    return with_scan_retry(c, [&] { return cd_crop_voxel_impl(c, points, stride, n, p, out_xyz, out_rgb, capacity, out_n_cropped, out_n_voxels); });
}
int cd_segment_plane(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, float coeff[4], int32_t* inliers, int capacity, int* out_n_inliers, int* out_iterations) {
    return with_scan_retry(c, [&] { return cd_segment_plane_impl(c, xyz, stride, n, p, coeff, inliers, capacity, out_n_inliers, out_iterations); });
}
int cd_surface_frame(cd_context* c, const void* xyz, size_t stride, int n, const float table_normal[3], int invert, const cd_params* p, cd_surface_frame_result* out) {
    return with_scan_retry(c, [&] { return cd_surface_frame_impl(c, xyz, stride, n, table_normal, invert, p, out); });
}
int cd_surface_batch(cd_context* c, const void* xyz, size_t stride, int points_per_frame, const int32_t* n_points, int n_frames, const float* table_normals, int invert, const cd_params* p, cd_surface_frame_result* out, int32_t* frame_status) {
    return with_scan_retry(c, [&] { return cd_surface_batch_impl(c, xyz, stride, points_per_frame, n_points, n_frames, table_normals, invert, p, out, frame_status); });
}
int cd_bbox_filter(cd_context* c, const void* xyz, size_t stride, int n, const double P[12], const int32_t rect[4], int32_t* out_indices, int capacity, int* out_n) {
    return with_scan_retry(c, [&] { return cd_bbox_filter_impl(c, xyz, stride, n, P, rect, out_indices, capacity, out_n); });
}
int cd_extract(cd_context* c, const void* points, size_t stride, int n, const int32_t* indices, int n_indices, int negative, void* out_points, int capacity, int* out_n) {
    return with_scan_retry(c, [&] { return cd_extract_impl(c, points, stride, n, indices, n_indices, negative, out_points, capacity, out_n); });
}
int cd_passthrough(cd_context* c, const void* points, size_t stride, int n, int field, double limit_min, double limit_max, int negative, void* out_points, int capacity, int* out_n) {
    return with_scan_retry(c, [&] { return cd_passthrough_impl(c, points, stride, n, field, limit_min, limit_max, negative, out_points, capacity, out_n); });
}
int cd_cluster(cd_context* c, const void* xyz, size_t stride, int n, const cd_params* p, int32_t* labels, int32_t* sizes, int sizes_capacity, int* out_k) {
    return with_scan_retry(c, [&] { return cd_cluster_impl(c, xyz, stride, n, p, labels, sizes, sizes_capacity, out_k); });
}
int cd_icp(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const cd_params* p, cd_cluster_result* out, float* aligned) {
    return with_scan_retry(c, [&] { return cd_icp_impl(c, slot, src_xyz, stride, n, p, out, aligned); });
}
int cd_shape_frames(cd_context* c, const void* xyz, size_t stride, const int32_t* offsets, int n_sets, cd_shape_frame* out) {
    return with_scan_retry(c, [&] { return cd_shape_frames_impl(c, xyz, stride, offsets, n_sets, out); });
}
int cd_ground_plane(cd_context* c, const void* points, size_t stride, int n, const cd_params* p, float coeff[4], void* out_records, int capacity, int* out_n, int* out_n_inliers) {
    return with_scan_retry(c, [&] { return cd_ground_plane_impl(c, points, stride, n, p, coeff, out_records, capacity, out_n, out_n_inliers); });
}
}  // extern "C"

// ---- cd_icp_solve_batch: the ICP step on its own (diagnostic; what cd_template_nearest is for the search) ----
// one wave = four records, one per row of 16 lanes: icp_step_row on a copy of the record's state, then icp_step on another
// copy by the row's first lane - the two solvers of one launch side by side, rows free to diverge
template <bool BOUNDED>
__global__ void __launch_bounds__(WAVE) k_icp_solve_batch(int k, const unsigned long long* __restrict__ sums, const int* __restrict__ n,
                                                           const IcpState* __restrict__ in, IcpParams prm, IcpState* __restrict__ out_row,
                                                           IcpState* __restrict__ out_lane, int* __restrict__ done) {
    __shared__ IcpState s_row[4], s_one[4];
    __shared__ unsigned long long s_sums[4][16];
    const int tid = (int)threadIdx.x, r = tid >> 4, l = tid & 15;
    const int rec = (int)blockIdx.x * 4 + r;
    if (rec >= k) return;   // (whole rows; no barrier below)
    if (l == 0) { s_row[r] = in[rec]; s_one[r] = in[rec]; }
    s_sums[r][l] = sums[(size_t)rec * 16 + l];
    const int nn = n[rec];
    RowLanes row(tid);
    RowLanes::V<unsigned long long> a;
    a.v = s_sums[r][l];
    const int d_row = icp_step_row<BOUNDED>(row, s_row[r], a, nn, prm);
    if (l == 0) {
        const int d_one = icp_step<BOUNDED>(s_one[r], s_sums[r], nn, prm);
        out_row[rec] = s_row[r];
        out_lane[rec] = s_one[r];
        done[2 * rec] = d_row;
        done[2 * rec + 1] = d_one;
    }
}
// sqrt_ge1 / rcp_ge1 against the compiler's IEEE sqrtf / division for EVERY float of their domains: x in [1, +inf] for the
// square root, |x| in [1, 2^126) for the reciprocal.  res: [0] square roots that differ, [1] the smallest such input's bits,
// [2], [3] the same for reciprocals
__global__ void __launch_bounds__(BLOCK) k_unary_exhaustive(unsigned long long* __restrict__ res) {
    unsigned long long bad_s = 0, bad_r = 0, first_s = ~0ull, first_r = ~0ull;
    const unsigned lo = 0x3f800000u, hi = 0x7f800000u, rcp_end = 0x7e800000u;   // 1.0f, +inf, 2^126
    for (unsigned long long b = lo + (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; b <= hi; b += (unsigned long long)gridDim.x * BLOCK) {
        const float x = __uint_as_float((unsigned)b);
        if (__float_as_uint(sqrt_ge1(x)) != __float_as_uint(sqrtf(x))) { bad_s += 1; first_s = first_s < b ? first_s : b; }
        if (b < rcp_end) {
            if (__float_as_uint(rcp_ge1(x)) != __float_as_uint(1.0f / x)) { bad_r += 1; first_r = first_r < b ? first_r : b; }
            const unsigned long long bn = b | 0x80000000ull;
            if (__float_as_uint(rcp_ge1(-x)) != __float_as_uint(1.0f / -x)) { bad_r += 1; first_r = first_r < bn ? first_r : bn; }
        }
    }
    if (bad_s) { atomicAdd(&res[0], bad_s); atomicMin(&res[1], first_s); }
    if (bad_r) { atomicAdd(&res[2], bad_r); atomicMin(&res[3], first_r); }
}

extern "C" int cd_icp_solve_batch(int k, const uint64_t* sums, const int32_t* n, const void* states_in, int max_iter, double trans_eps,
                                  double rel_mse, double rot_thr, double abs_mse, int bounded, void* states_row, void* states_lane,
                                  int32_t* done, uint64_t* unary) {
    static_assert(sizeof(IcpState) == 152, "the record layout cuboid_hip.h documents");
    if (k < 0 || (k > 0 && (!sums || !n || !states_in || !states_row || !states_lane || !done))) return CD_ERR_INVALID_ARG;
    unsigned long long *d_sums = nullptr, *d_res = nullptr;
    int *d_n = nullptr, *d_done = nullptr;
    IcpState *d_in = nullptr, *d_row = nullptr, *d_lane = nullptr;
    bool ok = true;
    auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; return ok; };
    if (k > 0) {
        const size_t kk = (size_t)k;
        if (chk(hipMalloc(&d_sums, kk * 128)) && chk(hipMalloc(&d_n, kk * 4)) && chk(hipMalloc(&d_done, kk * 8)) && chk(hipMalloc(&d_in, kk * sizeof(IcpState))) &&
            chk(hipMalloc(&d_row, kk * sizeof(IcpState))) && chk(hipMalloc(&d_lane, kk * sizeof(IcpState))) &&
            chk(hipMemcpy(d_sums, sums, kk * 128, hipMemcpyHostToDevice)) && chk(hipMemcpy(d_n, n, kk * 4, hipMemcpyHostToDevice)) &&
            chk(hipMemcpy(d_in, states_in, kk * sizeof(IcpState), hipMemcpyHostToDevice))) {
            IcpParams prm;
            std::memset(&prm, 0, sizeof(prm));
            prm.max_iter = max_iter; prm.trans_eps = trans_eps; prm.rel_mse = rel_mse; prm.rot_thr = rot_thr; prm.abs_mse = abs_mse;
            const int grid = (k + 3) / 4;
            if (bounded) hipLaunchKernelGGL(k_icp_solve_batch<true>, dim3(grid), dim3(WAVE), 0, 0, k, d_sums, d_n, d_in, prm, d_row, d_lane, d_done);
            else hipLaunchKernelGGL(k_icp_solve_batch<false>, dim3(grid), dim3(WAVE), 0, 0, k, d_sums, d_n, d_in, prm, d_row, d_lane, d_done);
            chk(hipGetLastError());
            chk(hipDeviceSynchronize());
            chk(hipMemcpy(states_row, d_row, kk * sizeof(IcpState), hipMemcpyDeviceToHost));
            chk(hipMemcpy(states_lane, d_lane, kk * sizeof(IcpState), hipMemcpyDeviceToHost));
            chk(hipMemcpy(done, d_done, kk * 8, hipMemcpyDeviceToHost));
        }
    }
    if (ok && unary) {
        const unsigned long long init[4] = {0ull, ~0ull, 0ull, ~0ull};
        if (chk(hipMalloc(&d_res, sizeof(init))) && chk(hipMemcpy(d_res, init, sizeof(init), hipMemcpyHostToDevice))) {
            hipLaunchKernelGGL(k_unary_exhaustive, dim3(4096), dim3(BLOCK), 0, 0, d_res);
            chk(hipGetLastError());
            chk(hipDeviceSynchronize());
            chk(hipMemcpy(unary, d_res, sizeof(init), hipMemcpyDeviceToHost));
        }
        if (ok) {
            unary[4] = CD_ROW_SQRT_GE1;   // does the library's icp_step_row use the short form (1) or the plain operation (0)
            unary[5] = CD_ROW_RCP_GE1;
        }
    }
    (void)hipFree(d_sums); (void)hipFree(d_n); (void)hipFree(d_done); (void)hipFree(d_in); (void)hipFree(d_row); (void)hipFree(d_lane); (void)hipFree(d_res);
    return ok ? CD_OK : CD_ERR_DEVICE;
}
