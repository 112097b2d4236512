// pose_info.hip - the pose information of ICP results (rule C23, k_pose_info.hip): the step of the fused batch call, the context's
// setting, the read-back of the per-cluster records, one pair as a call of its own, the rule as a host call and the covariance in
// the order of a ROS pose message
#include "context.hpp"

namespace {
// Examines `np` results into out[0 .. np): those that step 9 lets through become one item each, the items go to the device largest
// first, one launch on the context's stream fills their records (step 2's tau: tau_of) and one blocking copy brings them back;
// the others get their record here.  The grid is four workgroups a CU, capped like the ICP's own by CUBOID_ICP_MAX_WG (tests
// make one workgroup take many items with it).  May grow its buffers (which synchronises the stream); ends synchronised.
int run_pose_info(cd_context* c, const std::vector<ResultSpec>& specs, double max_range, double min_support, cd_pose_info* out) {
    const int np = (int)specs.size();
    if (np <= 0) return CD_OK;
    std::vector<PoseItem> items;
    for (int k = 0; k < np; ++k) {
        const ResultSpec& s = specs[(size_t)k];
        const bool slot_ok = s.slot >= 0 && s.slot < CD_MAX_TEMPLATES;
        const int pre = pose_pre_status(slot_ok ? c->tpl_m[s.slot] : 0, slot_ok ? c->tpl_faces[s.slot] : 0, s.T);
        if (pre != CD_OK) { pose_empty(s.n, pre, 0, 0, 0, 0, &out[k]); continue; }
        if (s.n <= 0) { pose_empty(s.n, CD_ERR_FEW_CORRESPONDENCES, 0, 0, 0, 0, &out[k]); continue; }   // (no point to look at)
        if (s.src_off < 0 || s.src_off + s.n > 0x7fffffffll) return fail(c, CD_ERR_CAPACITY, "a cluster's points lie beyond 2^31 records");
        PoseItem it;
        std::memset(&it, 0, sizeof(it));
        it.src_off = (int32_t)s.src_off; it.n = s.n; it.slot = s.slot; it.accepted = s.accepted; it.pair = k;
        std::memcpy(it.T, s.T, sizeof(it.T));
        std::memcpy(it.c0, c->tpl_centre[s.slot], sizeof(it.c0));
        it.length = c->tpl_length[s.slot];
        items.push_back(it);
    }
    const int n_items = (int)items.size();
    if (n_items == 0) return CD_OK;
    std::stable_sort(items.begin(), items.end(), [](const PoseItem& a, const PoseItem& b) { return a.n > b.n; });
    GROW(c, d_piitem, items.size()); GROW(c, h_piitem, items.size());
    GROW(c, d_pirec, (size_t)np); GROW(c, h_pirec, (size_t)np);
    GROW(c, d_piqueue, 1);
    std::memcpy(c->h_piitem.get(), items.data(), sizeof(PoseItem) * items.size());
    HIPCHK(c, hipMemcpyAsync(c->d_piitem, c->h_piitem, sizeof(PoseItem) * items.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_piqueue, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_pirec, 0, sizeof(cd_pose_info) * (size_t)np, c->stream));
    const int n_wg = c->tun.icp_max_wg > 0 ? std::min(c->tun.icp_max_wg, 4 * std::max(c->n_cu, 1)) : 4 * std::max(c->n_cu, 1);
    LAUNCH(c, launch_pose_info(c->stream, n_items, n_wg, c->d_piitem, c->d_lat, c->d_src0, tau_of(max_range), min_support, c->d_pirec, c->d_piqueue));
    HIPCHK(c, copy_sync(c, c->h_pirec, c->d_pirec, sizeof(cd_pose_info) * (size_t)np, hipMemcpyDeviceToHost));
    for (const PoseItem& it : items) {
        const cd_pose_info& r = c->h_pirec[it.pair];
        if (r.n_source != it.n || r.n_in < 0 || r.n_in > it.n) return fail(c, CD_ERR_DEVICE, "the pose-information kernel left an inconsistent record");
        out[it.pair] = r;
    }
    return CD_OK;
}

int pose_info_points_impl(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const float* T, double max_range, double min_support, int accepted,
                          cd_pose_info* out) {
    invalidate_last(c);
    if (int st = check_result_points(c, out != nullptr, slot, src_xyz, stride, n, T, pose_setting_ok(max_range, min_support),
                                     "max_range and min_support must be finite and > 0"))
        return st;
    if (int st = upload_points(c, src_xyz, stride, n, c->d_src0)) return st;
    const std::vector<ResultSpec> one{ResultSpec{0, n, slot, accepted ? 1 : 0, T}};
    return run_pose_info(c, one, max_range, min_support, out);
}

// 3 x 3 row-major product in double
void mat3_mul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
}  // namespace

namespace cd {
// The fused call's step between its ICP (every stage synchronised, c->last_clusters final; rule C21's step, when on, has run) and
// publish_last.  in: the clusters' points as extracted, d_src0 + orig_off[k] (size of the result), the slots' lattices in d_lat,
// every result's T, template_slot and accepted.  out: last_pose, one record per cluster (not valid before publish_last).
int stage_pose_info(cd_context* c, int ncl, const std::vector<long long>& orig_off) {
    c->last_pose.begin(ncl);
    if (ncl <= 0) return CD_OK;
    std::vector<cd_pose_info> rec((size_t)ncl);
    if (int st = run_pose_info(c, result_specs(c, ncl, orig_off), c->pose_range, c->pose_support, rec.data())) return st;
    for (int k = 0; k < ncl; ++k) c->last_pose.keep(k, rec[(size_t)k]);
    return CD_OK;
}
}  // namespace cd

extern "C" {
int cd_set_pose_info(cd_context* c, int enable, double max_range, double min_support) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!pose_setting_ok(max_range, min_support)) return fail(c, CD_ERR_INVALID_ARG, "max_range and min_support must be finite and > 0");
    c->pose_on = enable ? 1 : 0;
    c->pose_range = max_range;
    c->pose_support = min_support;
    return CD_OK;
}

int cd_get_pose_info(const cd_context* c, int* enable, double* max_range, double* min_support) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (enable) *enable = c->pose_on;
    if (max_range) *max_range = c->pose_range;
    if (min_support) *min_support = c->pose_support;
    return CD_OK;
}

int cd_pose_info_struct_size(void) { return (int)sizeof(cd_pose_info); }

int cd_get_cluster_pose_info(const cd_context* c, int frame, int first, int count, cd_pose_info* out) {
    return c ? c->last_pose.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_pose_info_points(cd_context* c, int slot, const void* src_xyz, size_t stride_bytes, int n, const float T[16], double max_range, double min_support,
                        int accepted, cd_pose_info* out) {
    return with_scan_retry(c, [&] { return pose_info_points_impl(c, slot, src_xyz, stride_bytes, n, T, max_range, min_support, accepted, out); });
}

int cd_pose_info_host(const void* tpl_xyz, size_t tpl_stride, int m, const void* src_xyz, size_t src_stride, int n, const float T[16], double max_range,
                      double min_support, int accepted, cd_pose_info* out) {
    if (!out || !T || m < 0 || n < 0 || (m > 0 && !tpl_xyz) || (n > 0 && !src_xyz) || tpl_stride < 12 || src_stride < 12) return CD_ERR_INVALID_ARG;
    if (!pose_setting_ok(max_range, min_support)) return CD_ERR_INVALID_ARG;
    std::vector<float> tpl, src = n > 0 ? gather_xyz(src_xyz, src_stride, n) : std::vector<float>();
    auto L = std::make_unique<IcpLattice>();
    L->nface = 0;
    if (m > 0) {
        tpl = gather_xyz(tpl_xyz, tpl_stride, m);
        lattice_detect(tpl.data(), m, L.get());
    }
    const int pre = pose_pre_status(m, L->nface, T);
    if (pre != CD_OK) { pose_empty(n, pre, 0, 0, 0, 0, out); return CD_OK; }
    std::vector<int> face_w((size_t)m, 0);
    pose_face_axes(*L, m, face_w.data());
    float c0[3];
    double length;
    pose_box(tpl.data(), m, c0, &length);
    long long S[POSE_NSUMS];
    int nf[3], bad;
    pose_passes_host(tpl.data(), m, face_w.data(), src.data(), n, T, tau_of(max_range), c0, S, nf, &bad);
    double ws[POSE_WS];
    pose_finish(n, bad, nf[0], nf[1], nf[2], S, c0[0], c0[1], c0[2], length, min_support, accepted ? 1 : 0, ws, out);
    return CD_OK;
}

int cd_pose_info_ros_covariance(const cd_pose_info* info, const float T[16], double out36[36]) {
    if (!info || !T || !out36) return CD_ERR_INVALID_ARG;
    // R_P = the transpose of T's rotation; J = [[-R_P [c0]x, -R_P], [-R_P, 0]]
    double R[9], cx[9] = {0.0, -info->centre[2], info->centre[1], info->centre[2], 0.0, -info->centre[0], -info->centre[1], info->centre[0], 0.0}, Rc[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)T[4 * j + i];
    mat3_mul(R, cx, Rc);
    double J[36] = {0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            J[6 * i + j] = -Rc[3 * i + j];
            J[6 * i + 3 + j] = -R[3 * i + j];
            J[6 * (3 + i) + j] = -R[3 * i + j];
        }
    double JS[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += J[6 * i + k] * info->covariance[6 * k + j];
            JS[6 * i + j] = acc;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += JS[6 * i + k] * J[6 * j + k];
            out36[6 * i + j] = acc;
        }
    return CD_OK;
}
}  // extern "C"
