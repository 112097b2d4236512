// icp_coarse.hip - coarse-to-fine ICP (rule C18; the two levels are run by stage_icp_levels, icp_stage.hip): the context's
// setting, the subsample as a host call and the read-back of the per-cluster stats
#include "context.hpp"

extern "C" {
int cd_set_icp_coarse(cd_context* c, int stride, int min_points) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (stride == 0) { c->coarse_stride = 0; return CD_OK; }   // off: min_points stays as it was
    if (!cd::coarse_setting_ok(stride, min_points))
        return cd::fail(c, CD_ERR_INVALID_ARG, "the coarse stride must be 0 (off) or in [2, 64], with min_points >= 3 * stride");
    // room for the coarse sets behind a stage's clusters (what the buffers hold is dead between calls, and the read-backs of the last
    // fused call that live in them go with it).  d_obj as well: the outlier filter (stage_outlier) swaps it with d_src, so whichever
    // of the two is the ICP source buffer of a call has the room
    const size_t need = cd::coarse_source_capacity((size_t)c->N * (size_t)c->F);
    if (c->d_src0.capacity() < need || c->d_src.capacity() < need || c->d_obj.capacity() < need || c->d_nn.capacity() < need || c->d_d2.capacity() < need) {
        hipSetDevice(c->device);
        cd::invalidate_last(c);
        GROW(c, d_src0, need); GROW(c, d_src, need); GROW(c, d_obj, need); GROW(c, d_nn, need); GROW(c, d_d2, need);
    }
    c->coarse_stride = stride;
    c->coarse_min = min_points;
    return CD_OK;
}

int cd_get_icp_coarse(const cd_context* c, int* stride, int* min_points) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (stride) *stride = c->coarse_stride;
    if (min_points) *min_points = c->coarse_min;
    return CD_OK;
}

int cd_icp_coarse_struct_size(void) { return (int)sizeof(cd_icp_coarse_stats); }

int cd_icp_coarse_subsample(int n, int stride, int min_points, int32_t* out_indices, int capacity) {
    return cd::coarse_subsample(n, stride, min_points, out_indices, capacity);
}

int cd_get_cluster_coarse_stats(const cd_context* c, int frame, int first, int count, cd_icp_coarse_stats* out) {
    return c ? c->last_coarse.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}
}  // extern "C"
