// outlier.hip - statistical outlier removal (rule C16, k_outlier.hip): the step of the fused batch call, the context's setting,
// the read-back of what the filter did and the filter as a call of its own
#include "context.hpp"

namespace cd {
// The fused call's step between stage_extract / sync_fs and stage_cluster_sync, skipped when the filter is off.
// in: d_obj + fs.n_o (max_no: the largest, as the host read it).  out: d_obj = the kept points of every frame in their order
// (compacted into d_src, which is free until the cluster stage, and the two buffers swapped: both hold F * N points), fs.n_o on
// the device and in the host's mirror, d_omap (rows of *map_pitch ints: a point's index in the filtered cloud or -1), d_orec and
// - by a transfer that the cluster stage's synchronisation covers - h_orec.  Scratch: d_d2 (every point's dist_i, rows of N).
// Issues two kernels and that transfer; may grow d_omap / d_orec / h_orec (which synchronises the stream); synchronises nothing else.
int stage_outlier(cd_context* c, int F, int max_no, int* map_pitch) {
    const int pitch = (std::max(max_no, 1) + 63) & ~63;
    *map_pitch = pitch;
    GROW(c, d_omap, (size_t)F * pitch);
    GROW(c, d_orec, (size_t)c->F);
    GROW(c, h_orec, (size_t)c->F);
    FrameState* mirror = c->tun.mirror_writes && c->tun.copy_kernels ? c->h_fs.get() : nullptr;
    LAUNCH(c, launch_outlier_knn(c->stream, c->d_obj, c->N, F, max_no, c->d_fs, c->outlier_k, c->d_d2, c->N));
    LAUNCH(c, launch_outlier_select(c->stream, c->d_obj, c->N, F, c->d_fs, mirror, c->d_d2, c->N, c->outlier_k, c->outlier_mul, c->outlier_neg,
                                    c->d_src, c->d_omap, pitch, nullptr, c->d_orec));
    std::swap(c->d_obj, c->d_src);
    HIPCHK(c, xfer(c, c->h_orec, c->d_orec, sizeof(OutlierRecord) * (size_t)F, hipMemcpyDeviceToHost));
    return CD_OK;
}
}  // namespace cd

namespace {
bool outlier_args_ok(int mean_k, double std_mul) { return mean_k >= 1 && mean_k <= OUTLIER_MAX_K && std::isfinite(std_mul); }

// One cloud as row 0: points to d_obj, dist to d_d2, map to d_omap, kept indices to d_cand, the record to d_orec
int outlier_filter_impl(cd_context* c, const void* xyz, size_t stride, int n, int mean_k, double std_mul, int negative, int32_t* out_indices,
                        int capacity, int* out_n, float* out_dist, double* stats) {
    invalidate_last(c);
    if ((!xyz && n > 0) || !out_n || n < 0 || capacity < 0 || (capacity > 0 && !out_indices) || stride < 12 || (stride & 3))
        return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (!outlier_args_ok(mean_k, std_mul)) return fail(c, CD_ERR_INVALID_ARG, "mean_k must be in 1 .. 63 and std_mul finite");
    *out_n = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0.0;
    if (n > c->N) return fail(c, CD_ERR_CAPACITY, "more points than the context capacity");
    if (n == 0) return CD_OK;
    const int pitch = (n + 63) & ~63;
    GROW(c, d_omap, (size_t)pitch);
    GROW(c, d_orec, (size_t)c->F);
    GROW(c, h_orec, (size_t)c->F);
    int st = upload_points(c, xyz, stride, n, c->d_obj);
    if (st) return st;
    std::memset(&c->h_fs[0], 0, sizeof(FrameState));
    c->h_fs[0].n_o = n;
    HIPCHK(c, xfer(c, c->d_fs, c->h_fs, sizeof(FrameState), hipMemcpyHostToDevice));
    LAUNCH(c, launch_outlier_knn(c->stream, c->d_obj, c->N, 1, n, c->d_fs, mean_k, c->d_d2, c->N));
    LAUNCH(c, launch_outlier_select(c->stream, c->d_obj, c->N, 1, c->d_fs, nullptr, c->d_d2, c->N, mean_k, std_mul, negative ? 1 : 0, nullptr, c->d_omap, pitch,
                                    c->d_cand, c->d_orec));
    HIPCHK(c, copy_sync(c, c->h_orec, c->d_orec, sizeof(OutlierRecord), hipMemcpyDeviceToHost));
    const OutlierRecord& r = c->h_orec[0];
    if (r.n_before != n || r.n_kept < 0 || r.n_kept > n) return fail(c, CD_ERR_DEVICE, "the outlier kernels left an inconsistent record");
    if (out_dist) HIPCHK(c, copy_sync(c, out_dist, c->d_d2, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    if (stats) { stats[0] = r.mean; stats[1] = r.stddev; stats[2] = r.threshold; }
    *out_n = r.n_kept;
    if (r.n_kept > capacity) return fail(c, CD_ERR_CAPACITY, "index capacity too small");
    if (r.n_kept > 0) HIPCHK(c, copy_sync(c, out_indices, c->d_cand, sizeof(int) * (size_t)r.n_kept, hipMemcpyDeviceToHost));
    return CD_OK;
}
}  // namespace

extern "C" {
int cd_set_outlier_filter(cd_context* c, int mean_k, double std_mul, int negative) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (mean_k != 0 && !outlier_args_ok(mean_k, std_mul)) return fail(c, CD_ERR_INVALID_ARG, "mean_k must be 0 (off) or in 1 .. 63, and std_mul finite");
    c->outlier_k = mean_k;
    if (mean_k != 0) { c->outlier_mul = std_mul; c->outlier_neg = negative ? 1 : 0; }
    return CD_OK;
}

int cd_get_outlier_filter(const cd_context* c, int* mean_k, double* std_mul, int* negative) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (mean_k) *mean_k = c->outlier_k;
    if (std_mul) *std_mul = c->outlier_mul;
    if (negative) *negative = c->outlier_neg;
    return CD_OK;
}

int cd_get_outlier_stats(const cd_context* c, int frame, int* n_before, int* n_removed, double* mean, double* stddev, double* threshold) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!c->last_outlier_ok || !c->last_clouds || frame < 0 || (size_t)frame >= c->last_outlier.size() || (size_t)frame + 1 >= c->last_first.size())
        return CD_ERR_INVALID_ARG;   // (const: no message; the call ran without the filter, has been invalidated, or had no such frame)
    const OutlierRecord& r = c->last_outlier[(size_t)frame];
    if (n_before) *n_before = r.n_before;
    if (n_removed) *n_removed = r.n_before - r.n_kept;
    if (mean) *mean = r.mean;
    if (stddev) *stddev = r.stddev;
    if (threshold) *threshold = r.threshold;
    return CD_OK;
}

int cd_outlier_filter(cd_context* c, const void* xyz, size_t stride_bytes, int n, int mean_k, double std_mul, int negative, int32_t* out_indices,
                      int capacity, int* out_n, float* out_dist, double stats[3]) {
    return with_scan_retry(c, [&] { return outlier_filter_impl(c, xyz, stride_bytes, n, mean_k, std_mul, negative, out_indices, capacity, out_n, out_dist, stats); });
}
}  // extern "C"
