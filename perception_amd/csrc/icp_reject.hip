// icp_reject.hip - median-distance correspondence rejection (rule C19, k_icp_reject.hip): the context's setting, the check every
// ICP entry point makes before it launches anything, the read-back of the per-cluster stats and the rule's arithmetic as a host call
#include <cmath>
#include <vector>

#include "context.hpp"

namespace cd {
int check_reject_mode(cd_context* c) {
    if (c->reject_factor == 0.0 || c->plane_weight == 0.0) return CD_OK;
    return fail(c, CD_ERR_INVALID_ARG, "median-distance rejection (cd_set_icp_median_rejection) and plane-weighted ICP (cd_set_icp_plane_weight) are both on: "
                                       "the plane-weighted step has no rejection; turn one of them off");
}
}  // namespace cd

extern "C" {
int cd_set_icp_median_rejection(cd_context* c, double factor) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (factor == 0.0) { c->reject_factor = 0.0; return CD_OK; }
    if (!(factor > 0.0) || !std::isfinite(factor)) return cd::fail(c, CD_ERR_INVALID_ARG, "the median factor must be 0 (off) or finite and > 0");   // (NaN fails)
    c->reject_factor = factor;
    return CD_OK;
}

int cd_get_icp_median_rejection(const cd_context* c, double* factor) {
    if (!c || !factor) return CD_ERR_INVALID_ARG;
    *factor = c->reject_factor;
    return CD_OK;
}

int cd_icp_reject_struct_size(void) { return (int)sizeof(cd_icp_reject_stats); }

int cd_get_cluster_reject_stats(const cd_context* c, int frame, int first, int count, cd_icp_reject_stats* out) {
    return c ? c->last_reject.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_icp_median_threshold(const float* d2, int n, double factor, float* median, double* thr) {
    if (!d2 || n < 1 || !(factor > 0.0) || !std::isfinite(factor)) return CD_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) if (cd::reject_key(d2[i]) > 0x7f800000u) return CD_ERR_INVALID_ARG;   // (NaN or signed: not a squared distance of rule C5)
    float m = 0.f;
    double t = 0.0;
    cd::reject_median_host(d2, (uint32_t)n, factor, &m, &t);
    if (median) *median = m;
    if (thr) *thr = t;
    return CD_OK;
}
}  // extern "C"
