// box_fit.hip - the box fit of clusters (rule C24, k_box_fit.hip): the step of the fused batch call, the context's setting, the
// read-back of the per-cluster records, several point sets as a call of their own, the rule as a host call and the template match
#include "context.hpp"

namespace {
struct BoxSpec {   // one cluster of a launch: its n points at pts + src_off, its frame's plane (have = 0: the frame has none)
    long long src_off;
    int n, have;
    float coeff[4];
};

// Issues the fit of `np` clusters: a cluster of fewer than three points gets its record in c->box_rec here, every other becomes one
// item with its frame's basis (steps 1 and 2, host arithmetic); the items go to the device largest first, one launch on the
// context's stream fills their records and one copy into the pinned mirror follows it on the stream.  The grid is four workgroups
// a CU, capped like the ICP's own by CUBOID_ICP_MAX_WG (tests make one workgroup take many items with it).  May grow its buffers
// (which synchronises the stream); synchronises nothing else: box_fit_collect ends the fit.
int box_fit_launch(cd_context* c, const std::vector<BoxSpec>& specs, const float4* pts, double band) {
    const int np = (int)specs.size();
    c->box_rec.assign((size_t)std::max(np, 1), cd_box_fit());
    c->box_items.clear();
    if (np <= 0) return CD_OK;
    std::vector<BoxItem>& items = c->box_items;
    for (int k = 0; k < np; ++k) {
        const BoxSpec& s = specs[(size_t)k];
        if (s.n < 3) { box_empty(s.n, 0, 0, CD_ERR_FEW_CORRESPONDENCES, 0, &c->box_rec[(size_t)k]); continue; }
        if (s.src_off < 0 || s.src_off + s.n > 0x7fffffffll) { items.clear(); return fail(c, CD_ERR_CAPACITY, "a cluster's points lie beyond 2^31 records"); }
        BoxItem it;
        std::memset(&it, 0, sizeof(it));
        it.src_off = (int32_t)s.src_off; it.n = s.n; it.rec = k; it.band_q = box_band_q(band);
        it.B = box_basis(s.coeff[0], s.coeff[1], s.coeff[2], s.coeff[3]);
        if (!s.have) it.B.have = 0;
        items.push_back(it);
    }
    const int n_items = (int)items.size();
    if (n_items == 0) return CD_OK;
    std::stable_sort(items.begin(), items.end(), [](const BoxItem& a, const BoxItem& b) { return a.n > b.n; });
    GROW(c, d_bfitem, items.size()); GROW(c, h_bfitem, items.size());
    GROW(c, d_bfrec, (size_t)np); GROW(c, h_bfrec, (size_t)np);
    GROW(c, d_bfqueue, 1);
    std::memcpy(c->h_bfitem.get(), items.data(), sizeof(BoxItem) * items.size());
    HIPCHK(c, hipMemcpyAsync(c->d_bfitem, c->h_bfitem, sizeof(BoxItem) * items.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_bfqueue, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_bfrec, 0, sizeof(cd_box_fit) * (size_t)np, c->stream));
    const int n_wg = c->tun.icp_max_wg > 0 ? std::min(c->tun.icp_max_wg, 4 * std::max(c->n_cu, 1)) : 4 * std::max(c->n_cu, 1);
    LAUNCH(c, launch_box_fit(c->stream, n_items, n_wg, c->d_bfitem, pts, c->d_bfrec, c->d_bfqueue));
    HIPCHK(c, hipMemcpyAsync(c->h_bfrec, c->d_bfrec, sizeof(cd_box_fit) * (size_t)np, hipMemcpyDeviceToHost, c->stream));
    return CD_OK;
}

// Ends the fit box_fit_launch issued: waits for the stream (a wait the caller's own synchronisation may already have made), checks
// the records the kernel left and puts them next to those the host wrote, in c->box_rec.
int box_fit_collect(cd_context* c) {
    if (c->box_items.empty()) return CD_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const BoxItem& it : c->box_items) {
        const cd_box_fit& r = c->h_bfrec[it.rec];
        if (r.n != it.n || r.n_top < 0 || r.n_top > it.n || r.hull_vertices < 0 || r.hull_vertices > PRISM_MAX_HULL) {
            c->box_items.clear();
            return fail(c, CD_ERR_DEVICE, "the box-fit kernel left an inconsistent record");
        }
        c->box_rec[(size_t)it.rec] = r;
    }
    c->box_items.clear();
    return CD_OK;
}

int box_fit_points_impl(cd_context* c, const float* coeff, const void* xyz, size_t stride, const int32_t* offsets, int n_sets, double band, cd_box_fit* out) {
    if (!coeff || !offsets || !out || n_sets <= 0 || stride < 12 || (stride & 3) || offsets[0] < 0) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    for (int i = 0; i < n_sets; ++i) if (offsets[i + 1] < offsets[i]) return fail(c, CD_ERR_INVALID_ARG, "offsets must ascend");
    if (!box_band_ok(band)) return fail(c, CD_ERR_INVALID_ARG, "band must be finite, > 0 and <= 64");
    const int base = offsets[0], total = offsets[n_sets] - base;
    if (total > 0 && !xyz) return fail(c, CD_ERR_INVALID_ARG, "null points");
    invalidate_last(c);
    GROW(c, d_bfpts, (size_t)std::max(total, 1));
    if (int st = upload_points(c, (const char*)xyz + (size_t)base * stride, stride, total, c->d_bfpts)) return st;
    std::vector<BoxSpec> specs((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) {
        BoxSpec& s = specs[(size_t)i];
        s.src_off = offsets[i] - base; s.n = offsets[i + 1] - offsets[i]; s.have = 1;
        std::memcpy(s.coeff, coeff + 4 * (size_t)i, sizeof(s.coeff));
    }
    if (int st = box_fit_launch(c, specs, c->d_bfpts, band)) return st;
    if (int st = box_fit_collect(c)) return st;
    std::memcpy(out, c->box_rec.data(), sizeof(cd_box_fit) * (size_t)n_sets);
    return CD_OK;
}
}  // namespace

namespace cd {
// The fused call's step right after the cluster hand-over (batch_clusters), ahead of the ICP: the clusters as clustered - after the
// table prism and the outlier filter when those are on.  in: every cluster's points as extracted, size[k] of them at d_src0 +
// orig_off[k] (every extraction round has been issued), the frames' planes as the host's mirrors hold them since the cluster
// stage's synchronisation.  Issues the launch and the copy of the records; the records are in c->box_rec after
// stage_box_fit_collect, which the caller makes at once when the selection needs them for the ICP's planning and behind the ICP
// (whose stages end synchronised) otherwise.
int stage_box_fit(cd_context* c, int F, const std::vector<int>& first, const std::vector<int>& size, const std::vector<long long>& orig_off) {
    const int ncl = first.empty() ? 0 : first.back();
    c->last_box.begin(ncl);
    std::vector<BoxSpec> specs((size_t)std::max(ncl, 0));
    for (int f = 0; f < F; ++f)
        for (int k = first[(size_t)f]; k < first[(size_t)f + 1]; ++k) {
            BoxSpec& s = specs[(size_t)k];
            s.src_off = orig_off[(size_t)k]; s.n = size[(size_t)k]; s.have = c->h_have[f] ? 1 : 0;
            const float4 m = c->h_model[f];
            s.coeff[0] = m.x; s.coeff[1] = m.y; s.coeff[2] = m.z; s.coeff[3] = m.w;
        }
    return box_fit_launch(c, specs, c->d_src0, c->box_band);
}

// out: c->box_rec and last_box, one record per cluster (not valid before publish_last).  With the selection on (cd_set_box_select)
// every CD_OK record carries cd_box_fit_match's answer over the loaded slots.
int stage_box_fit_collect(cd_context* c, int ncl) {
    if (int st = box_fit_collect(c)) return st;
    if (c->box_select_on) {
        uint32_t mask = 0u;
        for (int s = 0; s < CD_MAX_TEMPLATES; ++s) if (c->tpl_m[s] > 0) mask |= 1u << s;
        for (int k = 0; k < ncl; ++k) {
            cd_box_fit& r = c->box_rec[(size_t)k];
            if (r.status == CD_OK) box_match(r.dims, c->box_slot_dims, mask, c->box_tolerance, &r.match_slot, &r.match_cost);
        }
    }
    for (int k = 0; k < ncl; ++k) c->last_box.keep(k, c->box_rec[(size_t)k]);
    return CD_OK;
}
}  // namespace cd

extern "C" {
int cd_set_box_fit(cd_context* c, int enable, double band) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!enable) { c->box_on = 0; c->box_select_on = 0; return CD_OK; }   // (off: the band is not looked at and stays; the selection needs the fit)
    if (!box_band_ok(band)) return fail(c, CD_ERR_INVALID_ARG, "band must be finite, > 0 and <= 64");
    c->box_on = 1;
    c->box_band = band;
    return CD_OK;
}

int cd_get_box_fit(const cd_context* c, int* enable, double* band) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (enable) *enable = c->box_on;
    if (band) *band = c->box_band;
    return CD_OK;
}

int cd_set_box_select(cd_context* c, int enable, const double slot_dims[CD_MAX_TEMPLATES][3], double tolerance) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!enable) { c->box_select_on = 0; return CD_OK; }
    if (!c->box_on) return fail(c, CD_ERR_INVALID_ARG, "the selection needs the box fit on (cd_set_box_fit)");
    if (!slot_dims || !(tolerance >= 0.0) || !std::isfinite(tolerance)) return fail(c, CD_ERR_INVALID_ARG, "slot_dims is NULL, or the tolerance is not finite or negative");
    for (int s = 0; s < CD_MAX_TEMPLATES; ++s)
        for (int j = 0; j < 3; ++j) if (!std::isfinite(slot_dims[s][j])) return fail(c, CD_ERR_INVALID_ARG, "slot_dims holds a non-finite value");
    c->box_select_on = 1;
    std::memcpy(c->box_slot_dims, slot_dims, sizeof(c->box_slot_dims));
    c->box_tolerance = tolerance;
    return CD_OK;
}

int cd_get_box_select(const cd_context* c, int* enable, double slot_dims[CD_MAX_TEMPLATES][3], double* tolerance) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (enable) *enable = c->box_select_on;
    if (slot_dims) std::memcpy(slot_dims, c->box_slot_dims, sizeof(c->box_slot_dims));
    if (tolerance) *tolerance = c->box_tolerance;
    return CD_OK;
}

int cd_box_fit_struct_size(void) { return (int)sizeof(cd_box_fit); }

int cd_get_cluster_box_fits(const cd_context* c, int frame, int first, int count, cd_box_fit* out) {
    return c ? c->last_box.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_box_fit_points(cd_context* c, const float* coeff, const void* xyz, size_t stride_bytes, const int32_t* offsets, int n_sets, double band, cd_box_fit* out) {
    return with_scan_retry(c, [&] { return box_fit_points_impl(c, coeff, xyz, stride_bytes, offsets, n_sets, band, out); });
}

int cd_box_fit_host(const float coeff[4], const void* xyz, size_t stride_bytes, int n, double band, cd_box_fit* out) {
    if (!coeff || !out || n < 0 || (n > 0 && !xyz) || stride_bytes < 12 || !box_band_ok(band)) return CD_ERR_INVALID_ARG;
    box_fit_host(coeff, xyz, stride_bytes, n, band, 1, out);
    return CD_OK;
}

int cd_box_fit_match(const double dims[3], const double slot_dims[CD_MAX_TEMPLATES][3], uint32_t loaded_mask, double tolerance, int32_t* slot, double* cost) {
    if (!dims || !slot_dims || !slot || !cost || !(tolerance >= 0.0)) return CD_ERR_INVALID_ARG;
    box_match(dims, slot_dims, loaded_mask, tolerance, slot, cost);
    return CD_OK;
}
}  // extern "C"
