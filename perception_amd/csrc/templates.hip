// templates.hip - the process-wide template cache, cd_set_template and the lattice and nearest-neighbour entries.
//
// Everything cd_set_template derives from the template's points is device-independent host work (template_prep.hpp): it is
// done once per distinct template and shared by every context of the process (bench.py keeps three contexts per GPU; the
// reference re-reads and re-indexes the template for every frame, icp.cpp:159).  The cache is process-wide, keyed on m plus the
// raw bytes, and keeps the 16 newest entries.
// (cell_factor is tuning only and not part of the key: a cached template keeps the factor it was prepared with)
#include "context.hpp"

namespace {
// (the cache and its mutex are this function's statics: one instance, as the function is defined in this unit only)
std::shared_ptr<const PreparedTemplate> prepared_template_cached(const void* xyz, size_t stride, int m, float cell_factor) {
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    static std::mutex mu;
    static std::vector<std::shared_ptr<const PreparedTemplate>> cache;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto& e : cache)
            if (e->m == m && std::memcmp(e->xyz.data(), raw.data(), raw.size() * sizeof(float)) == 0) return e;
    }
    std::shared_ptr<const PreparedTemplate> P = prepare_template(raw.data(), m, cell_factor);
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.push_back(P);
    return P;
}

// copies a prepared template into the context's template arena at point offset `off` (a multiple of 64)
int upload_template(cd_context* c, int slot, int off, const PreparedTemplate& P) {
    const int nrun = P.m_pad / ICP_SUB;
    HIPCHK(c, copy_sync(c, c->d_tpl + off, P.cell_pts.data(), sizeof(float4) * (size_t)P.m_pad, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tlo + off / ICP_SUB, P.cell_lo.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_thi + off / ICP_SUB, P.cell_hi.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tplk + off, P.kd_pts.data(), sizeof(float4) * (size_t)P.m_pad, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_tlok + off / ICP_SUB, P.kd_lo.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_thik + off / ICP_SUB, P.kd_hi.data(), sizeof(float4) * (size_t)nrun, hipMemcpyHostToDevice));
    if (!P.kdmap.empty())
        HIPCHK(c, copy_sync(c, c->d_kdmap + off, P.kdmap.data(), sizeof(unsigned short) * P.kdmap.size(), hipMemcpyHostToDevice));
    IcpGrid grid = P.grid;
    grid.cell_off = slot * ICP_CELL_STRIDE;
    if (!P.cell_start.empty())
        HIPCHK(c, copy_sync(c, c->d_tcell + grid.cell_off, P.cell_start.data(), sizeof(unsigned short) * P.cell_start.size(), hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_grid + slot, &grid, sizeof(grid), hipMemcpyHostToDevice));
    c->tpl_off[slot] = off;
    c->tpl_m[slot] = P.m;
    c->tpl_gridded[slot] = grid.ncell > 0;
    c->tpl_big[slot] = P.big_ok;
    HIPCHK(c, copy_sync(c, c->d_super + slot, &P.super, sizeof(IcpSuper), hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->d_lat + slot, &P.lat, sizeof(IcpLattice), hipMemcpyHostToDevice));
    c->tpl_faces[slot] = P.lat.nface;
    c->tpl_frame[slot] = P.frame;
    pose_box(P.xyz.data(), P.m, c->tpl_centre[slot], &c->tpl_length[slot]);   // rule C23, step 3
    c->tframe_dirty = true;   // (rule C13's slot table: uploaded by the next CD_GUESS_CLUSTER stage)
    return CD_OK;
}
}  // namespace

extern "C" {
int cd_set_template(cd_context* c, int slot, const void* xyz, size_t stride, int m) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (slot < 0 || slot >= CD_MAX_TEMPLATES || !xyz || m <= 0 || stride < 12) return fail(c, CD_ERR_INVALID_ARG, "bad template arguments");
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float cell_factor = 2.0f;
    if (const char* e = std::getenv("CUBOID_ICP_CELL_FACTOR")) cell_factor = (float)std::atof(e);   // tuning only
    std::shared_ptr<const PreparedTemplate> P = prepared_template_cached(xyz, stride, m, cell_factor);
    // a slot is re-used in place when the new template fits its space, appended otherwise; when the arena is full the
    // live slots are packed again (the space of replaced templates is reclaimed) before giving up
    const int old_pad = c->tpl_prep[slot] ? c->tpl_prep[slot]->m_pad : 0;
    if (old_pad >= P->m_pad) {
        c->tpl_prep[slot] = P;
        return upload_template(c, slot, c->tpl_off[slot], *P);
    }
    if (c->tpl_used + P->m_pad <= c->tpl_cap) {
        const int off = c->tpl_used;
        c->tpl_used += P->m_pad;
        c->tpl_prep[slot] = P;
        return upload_template(c, slot, off, *P);
    }
    long long total = P->m_pad;
    for (int k = 0; k < CD_MAX_TEMPLATES; ++k) if (k != slot && c->tpl_prep[k]) total += c->tpl_prep[k]->m_pad;
    if (total > c->tpl_cap) return fail(c, CD_ERR_CAPACITY, "template storage exhausted");
    c->tpl_prep[slot] = P;
    int off = 0;
    for (int k = 0; k < CD_MAX_TEMPLATES; ++k) {
        if (!c->tpl_prep[k]) continue;
        if (int ust = upload_template(c, k, off, *c->tpl_prep[k])) return ust;
        off += c->tpl_prep[k]->m_pad;
    }
    c->tpl_used = off;
    return CD_OK;
}

int cd_template_lattice_faces(const cd_context* c, int slot) {
    if (!c || slot < 0 || slot >= CD_MAX_TEMPLATES) return CD_ERR_INVALID_ARG;
    if (c->tpl_m[slot] <= 0) return CD_ERR_NO_TEMPLATE;
    return c->tpl_faces[slot];
}

int cd_lattice_detect(const void* xyz, size_t stride, int m, int32_t* out) {
    if (!xyz || m <= 0 || stride < 12) return CD_ERR_INVALID_ARG;
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    auto L = std::make_unique<IcpLattice>();
    lattice_detect(raw.data(), m, L.get());
    for (int f = 0; out && f < L->nface; ++f) {
        const int w = L->w[f], u = L->fast[f], v = 3 - w - u;
        const int32_t row[5] = {w, u, L->base[f], L->n[u], L->n[v]};
        std::memcpy(out + 5 * f, row, sizeof(row));
    }
    return L->nface;
}

int cd_lattice_axes(const void* xyz, size_t stride, int m, int32_t* out_axis_face, float* out_axis_c) {
    if (!xyz || m <= 0 || stride < 12) return CD_ERR_INVALID_ARG;
    const std::vector<float> raw = gather_xyz(xyz, stride, m);
    auto L = std::make_unique<IcpLattice>();
    lattice_detect(raw.data(), m, L.get());
    if (L->nface == 0) lattice_classify_axes(L.get());   // (not a lattice: the "none" values)
    if (out_axis_face) std::memcpy(out_axis_face, L->axis_face, sizeof(L->axis_face));
    if (out_axis_c) std::memcpy(out_axis_c, L->axis_c, sizeof(L->axis_c));
    return L->axes_distinct;
}

int cd_template_nearest(cd_context* c, int slot, const void* queries, size_t stride, int n, int32_t* out_index, float* out_d2) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (slot < 0 || slot >= CD_MAX_TEMPLATES || !queries || n <= 0 || stride < 12 || !out_index || !out_d2) return fail(c, CD_ERR_INVALID_ARG, "bad arguments");
    if (c->tpl_m[slot] <= 0) return fail(c, CD_ERR_NO_TEMPLATE, "template slot empty");
    if (c->tpl_faces[slot] <= 0) return fail(c, CD_ERR_INVALID_ARG, "the slot's template is not a lattice: its nearest-neighbour searches only exist inside the ICP kernels");
    if ((long long)n > (long long)c->N * c->F) return fail(c, CD_ERR_CAPACITY, "more queries than the context holds points");
    hipSetDevice(c->device);
    invalidate_last(c);
    int st = upload_points(c, queries, stride, n, c->d_src0);
    if (st) return st;
    LAUNCH(c, launch_lat_nn(c->stream, c->d_lat + slot, c->d_src0, n, c->d_nn, c->d_d2));
    HIPCHK(c, copy_sync(c, out_index, c->d_nn, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, copy_sync(c, out_d2, c->d_d2, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return CD_OK;
}
}  // extern "C"
