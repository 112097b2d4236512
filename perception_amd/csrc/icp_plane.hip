// icp_plane.hip - plane-weighted ICP for lattice templates (rule C17, k_icp_plane.hip): the context's setting, the check every
// ICP entry point makes before it launches anything, the read-back of the per-cluster counters and the solve as a host call
#include "context.hpp"

namespace cd {
int check_plane_templates(cd_context* c, int slot) {
    if (c->plane_weight == 0.0) return CD_OK;
    for (int s = 0; s < CD_MAX_TEMPLATES; ++s) {
        if (slot >= 0 && s != slot) continue;
        if (c->tpl_m[s] > 0 && c->tpl_faces[s] <= 0) {
            std::snprintf(c->err, sizeof(c->err), "plane-weighted ICP (cd_set_icp_plane_weight) is on and the template of slot %d is not a lattice", s);
            return CD_ERR_INVALID_ARG;
        }
    }
    return CD_OK;
}
}  // namespace cd

extern "C" {
int cd_set_icp_plane_weight(cd_context* c, double tangent_weight, double switch_distance) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (tangent_weight == 0.0) { c->plane_weight = 0.0; return CD_OK; }   // off: the switch distance stays as it was
    if (!(tangent_weight >= CD_ICP_PLANE_WEIGHT_MIN && tangent_weight <= 1.0))
        return cd::fail(c, CD_ERR_INVALID_ARG, "the tangent weight must be 0 (off) or in [1/1024, 1]");
    if (!(switch_distance >= 0.0)) return cd::fail(c, CD_ERR_INVALID_ARG, "the switch distance must be >= 0 (or +inf)");   // (NaN fails)
    c->plane_weight = tangent_weight;
    c->plane_switch = switch_distance;
    return CD_OK;
}

int cd_get_icp_plane_weight(const cd_context* c, double* tangent_weight, double* switch_distance) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (tangent_weight) *tangent_weight = c->plane_weight;
    if (switch_distance) *switch_distance = c->plane_switch;
    return CD_OK;
}

int cd_get_cluster_plane_stats(const cd_context* c, int frame, int first, int count, cd_icp_plane_stats* out) {
    return c ? c->last_plane.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_icp_plane_solve_host(const int64_t sums[28], int n, float T[16], int32_t* singular) {
    if (!sums || !T) return CD_ERR_INVALID_ARG;
    long long A[cd::PLANE_NSUMS];
    for (int i = 0; i < cd::PLANE_NSUMS; ++i) A[i] = (long long)sums[i];
    const int s = cd::plane_solve(A, n, T);
    if (singular) *singular = s;
    return CD_OK;
}
}  // extern "C"
