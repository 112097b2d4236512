// icp_recip.hip - reciprocal correspondences (rule C22, k_icp_recip.hip): the context's setting, the check every ICP entry point
// makes before it launches anything, the read-back of the per-cluster stats and the rule's arithmetic as a host call
#include <cmath>
#include <vector>

#include "context.hpp"

namespace cd {
int check_recip_mode(cd_context* c) {
    if (!c->recip_on) return CD_OK;
    if (c->plane_weight != 0.0)
        return fail(c, CD_ERR_INVALID_ARG, "reciprocal correspondences (cd_set_icp_reciprocal) and plane-weighted ICP (cd_set_icp_plane_weight) are both on: "
                                           "the plane-weighted step has no rejection; turn one of them off");
    if (c->reject_factor != 0.0)
        return fail(c, CD_ERR_INVALID_ARG, "reciprocal correspondences (cd_set_icp_reciprocal) and median-distance rejection (cd_set_icp_median_rejection) are both on: "
                                           "the two are not composed; turn one of them off");
    return CD_OK;
}
}  // namespace cd

extern "C" {
int cd_set_icp_reciprocal(cd_context* c, int on) {
    if (!c) return CD_ERR_INVALID_ARG;
    c->recip_on = on ? 1 : 0;
    return CD_OK;
}

int cd_get_icp_reciprocal(const cd_context* c, int* on) {
    if (!c || !on) return CD_ERR_INVALID_ARG;
    *on = c->recip_on;
    return CD_OK;
}

int cd_icp_recip_struct_size(void) { return (int)sizeof(cd_icp_recip_stats); }

int cd_get_cluster_recip_stats(const cd_context* c, int frame, int first, int count, cd_icp_recip_stats* out) {
    return c ? c->last_recip.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_icp_reciprocal_mask(const void* src_xyz, size_t src_stride, int n, const void* tpl_xyz, size_t tpl_stride, int m, float d2_max, int32_t* nn, float* d2,
                           uint8_t* keep) {
    if (!src_xyz || !tpl_xyz || !keep || n < 1 || m < 1 || src_stride < 12 || (src_stride & 3) || tpl_stride < 12 || (tpl_stride & 3) || !(d2_max >= 0.f))
        return CD_ERR_INVALID_ARG;   // (a NaN bound fails the comparison)
    const float* src = (const float*)src_xyz;
    const float* tpl = (const float*)tpl_xyz;
    std::vector<int32_t> j((size_t)n);
    std::vector<float> d((size_t)n);
    for (int i = 0; i < n; ++i) {
        const float* x = src + (size_t)i * (src_stride / 4);
        j[(size_t)i] = cd::recip_forward_host(tpl, tpl_stride / 4, m, x[0], x[1], x[2], &d[(size_t)i]);
    }
    const int n0 = cd::recip_mask_host(src, src_stride / 4, n, tpl, tpl_stride / 4, d2_max, j.data(), d.data(), keep);
    if (nn) std::copy(j.begin(), j.end(), nn);
    if (d2) std::copy(d.begin(), d.end(), d2);
    return n0;
}
}  // extern "C"
