// template_prep.hpp - everything cd_set_template derives from a template's points: host work without a HIP runtime call, so
// that the byte layouts the ICP search kernels depend on can be built, checked and sanitized on a CPU (template_prep_check.cpp).
// prepare_template, at the end, is the list of what a prepared template consists of.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "common.hpp"
#include "shape_frame_math.hpp"

namespace cd {

struct PreparedTemplate {
    int m = 0, m_pad = 0;
    std::vector<float> xyz;                              // the caller's points (cache key check)
    std::vector<float4> cell_pts, cell_lo, cell_hi;      // layout 1: sorted by grid cell; boxes of its runs of 64
    std::vector<float4> kd_pts, kd_lo, kd_hi;            // layout 2: k-d patches of 64; their boxes
    std::vector<unsigned short> kdmap;                   // patch order -> cell-sorted position (LDS-resident templates)
    std::vector<unsigned short> cell_start;              // grid start table (LDS-resident templates)
    IcpGrid grid;                                        // cell_off is set per slot at upload
    IcpSuper super;                                      // second box level of a template that does not fit LDS (n = 0: none)
    bool big_ok = false;                                 // k_icp_pipe_big can search it
    IcpLattice lat;                                      // nface > 0: the template is a union of axis-aligned lattices (k_icp_lat.hip)
    ShapeFrame frame;                                    // rule C13: the template's principal frame (shape_frame_host)
};

inline std::vector<float> gather_xyz(const void* xyz, size_t stride, int n) {
    std::vector<float> raw((size_t)n * 3);
    for (int i = 0; i < n; ++i) std::memcpy(&raw[3 * (size_t)i], (const char*)xyz + (size_t)i * stride, 12);
    return raw;
}

// rule C13 steps 1-4 on the host: the sums as the device forms them (fixq = llrint(ldexp(v, 32)), round to nearest even), then
// shape_frame_math.hpp
inline void shape_frame_host(const void* xyz, size_t stride, int n, ShapeFrame* out) {
    if (n > SHAPE_N_MAX) { shape_empty(n, SHAPE_ERR_CAPACITY, out); return; }
    auto point = [&](int i, float v[3]) { std::memcpy(v, (const char*)xyz + (size_t)i * stride, 12); };
    uint64_t S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool bad = false;
    for (int i = 0; i < n; ++i) {
        float v[3];
        point(i, v);
        bad = bad || !shape_coord_ok(v[0], v[1], v[2]);
        if (bad) break;
        const float t[9] = {v[0], v[1], v[2], v[0] * v[0], v[0] * v[1], v[0] * v[2], v[1] * v[1], v[1] * v[2], v[2] * v[2]};
        for (int k = 0; k < 9; ++k) S[k] += (uint64_t)std::llrint(std::ldexp((double)t[k], FIX_SHIFT));
    }
    if (bad) { shape_empty(n, SHAPE_ERR_INVALID, out); return; }
    if (n < 3) { shape_empty(n, SHAPE_ERR_FEW, out); return; }
    long long T[9];
    for (int k = 0; k < 9; ++k) T[k] = (long long)S[k];
    shape_empty(n, SHAPE_OK, out);
    shape_solve(T, n, out);
    const double inf = std::numeric_limits<double>::infinity();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int i = 0; i < n; ++i) {
        float v[3];
        double q[3];
        point(i, v);
        shape_project(out->mean, out->axes, v[0], v[1], v[2], q);
        for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], q[a]); hi[a] = std::fmax(hi[a], q[a]); }
    }
    for (int a = 0; a < 3; ++a) { out->lo[a] = lo[a] + 0.0; out->hi[a] = hi[a] + 0.0; }   // (a zero extent is stored as +0)
}

// the axis tables of a lattice as the kernel reads them; false: too many entries, or a table that is not near-uniform
inline bool lattice_tables(const std::vector<float> tabs[3], IcpLattice* out) {
    int ntab = 0;
    for (int a = 0; a < 3; ++a) {
        const std::vector<float>& T = tabs[a];
        const int n = (int)T.size();
        out->toff[a] = ntab;
        if (n == 0) {   // no face varies along this axis: a one-entry table, so that the kernel treats every axis alike (never read by a face)
            if (ntab + 1 > LAT_MAX_TAB) return false;
            out->n[a] = 1; out->noi[a] = 0.f; out->inv[a] = 1.f;
            out->tab[ntab++] = make_float4(-INFINITY, 0.f, INFINITY, 0.f);
            continue;
        }
        out->n[a] = n;
        if (ntab + n > LAT_MAX_TAB) return false;
        const double step = ((double)T[(size_t)n - 1] - (double)T[0]) / (double)(n - 1);
        for (int i = 0; i < n; ++i)   // uniform to 1/16 of a step: the index guess of lat_axis is then at most one entry off
            if (!(std::fabs((double)T[(size_t)i] - ((double)T[0] + i * step)) <= step / 16.0)) return false;
        out->noi[a] = (float)(-(double)T[0] / step);
        out->inv[a] = (float)(1.0 / step);
        for (int i = 0; i < n; ++i)
            out->tab[ntab + i] = make_float4(i > 0 ? T[(size_t)i - 1] : -INFINITY, T[(size_t)i], i + 1 < n ? T[(size_t)i + 1] : INFINITY, 0.f);
        ntab += n;
    }
    out->ntab = ntab;
    return true;
}

// Is the template what make_cuboid.py writes (mkc.py:38-55) - faces one after the other, each the Cartesian product of two of
// three shared, ascending, near-uniform axis tables at a constant third coordinate, first axis fastest?  Verified bit by bit
// against the points; anything else (a point moved, a row missing, the object templates) leaves nface = 0.
inline void lattice_detect(const float* xyz, int m, IcpLattice* out) {
    std::memset(out, 0, sizeof(*out));
    struct Face { int w, u, v, base, nu, nv; float c; };
    std::vector<Face> faces;
    std::vector<float> tabs[3];
    auto P = [&](int i, int a) { return xyz[3 * (size_t)i + a]; };
    for (int i = 0; i < 3 * m; ++i) if (!std::isfinite(xyz[i])) return;
    int pos = 0;
    while (pos < m) {
        if ((int)faces.size() >= LAT_MAX_FACES || pos + 1 >= m) return;
        int u = -1;
        for (int a = 0; a < 3; ++a)
            if (P(pos + 1, a) != P(pos, a)) { if (u >= 0) return; u = a; }
        if (u < 0) return;
        int nu = 1;   // first row: only u moves, ascending
        while (pos + nu < m && P(pos + nu, u) > P(pos + nu - 1, u) && P(pos + nu, (u + 1) % 3) == P(pos, (u + 1) % 3) &&
               P(pos + nu, (u + 2) % 3) == P(pos, (u + 2) % 3)) ++nu;
        if (nu < 2 || pos + nu >= m) return;
        int v = -1;
        for (int a = 0; a < 3; ++a)
            if (P(pos + nu, a) != P(pos, a)) { if (v >= 0 || a == u) return; v = a; }
        if (v < 0) return;
        const int w = 3 - u - v;
        int nv = 1;   // further rows: the same u values, v constant within the row and ascending from row to row, w constant
        while (pos + (nv + 1) * nu <= m) {
            const int r = pos + nv * nu;
            bool ok = P(r, v) > P(r - nu, v);
            for (int i = 0; i < nu && ok; ++i) ok = P(r + i, u) == P(pos + i, u) && P(r + i, v) == P(r, v) && P(r + i, w) == P(pos, w);
            if (!ok) break;
            ++nv;
        }
        if (nv < 2) return;
        std::vector<float> U((size_t)nu), V((size_t)nv);
        for (int i = 0; i < nu; ++i) U[(size_t)i] = P(pos + i, u);
        for (int j = 0; j < nv; ++j) V[(size_t)j] = P(pos + j * nu, v);
        const std::pair<int, std::vector<float>*> both[2] = {{u, &U}, {v, &V}};
        for (const auto& av : both) {   // one table per axis, shared by every face that varies along it
            if (tabs[av.first].empty()) tabs[av.first] = *av.second;
            else if (tabs[av.first] != *av.second) return;
        }
        faces.push_back(Face{w, u, v, pos, nu, nv, P(pos, w)});
        pos += nu * nv;
    }
    if (!lattice_tables(tabs, out)) { std::memset(out, 0, sizeof(*out)); return; }
    for (size_t f = 0; f < faces.size(); ++f) {
        out->w[f] = faces[f].w; out->fast[f] = faces[f].u; out->base[f] = faces[f].base; out->c[f] = faces[f].c;
        out->m0[f] = faces[f].w == 0 ? ~0u : 0u; out->m1[f] = faces[f].w == 1 ? ~0u : 0u; out->m2[f] = faces[f].w == 2 ? ~0u : 0u;
    }
    for (size_t f = faces.size(); f < (size_t)LAT_MAX_FACES; ++f) { out->w[f] = 2; out->m2[f] = ~0u; out->c[f] = std::numeric_limits<float>::quiet_NaN(); }   // (see IcpLattice::m0)
    out->nface = (int)faces.size();
    lattice_classify_axes(out);
}

// ---- the two sorted layouts: the steps of prepare_template ------------------------------------------------------------
namespace tprep {

struct TP { float x, y, z; int oi; int cid; };   // a template point, its original index and its grid cell
struct Box { float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}; };
typedef std::vector<std::pair<int, int>> Ranges;   // [lo, hi) of stored points
inline float int_bits(int i) { float f; std::memcpy(&f, &i, 4); return f; }

// exact float min/max of the points [first, last); finite_only: a coordinate that is not finite does not count
inline Box box_of_points(const TP* first, const TP* last, bool finite_only = false) {
    Box b;
    for (const TP* p = first; p < last; ++p) {
        const float v[3] = {p->x, p->y, p->z};
        for (int a = 0; a < 3; ++a)
            if (!finite_only || std::isfinite(v[a])) { b.mn[a] = std::fmin(b.mn[a], v[a]); b.mx[a] = std::fmax(b.mx[a], v[a]); }
    }
    return b;
}
// union of the run boxes r0 .. r1 - 1 of one layout (of no run: +-FLT_MAX), as the device records hold a box
inline void box_of_runs(const std::vector<float4>& lo, const std::vector<float4>& hi, int r0, int r1, float out_lo[4], float out_hi[4]) {
    Box b;
    for (int r = r0; r < r1; ++r) {
        const float lo3[3] = {lo[(size_t)r].x, lo[(size_t)r].y, lo[(size_t)r].z};
        const float hi3[3] = {hi[(size_t)r].x, hi[(size_t)r].y, hi[(size_t)r].z};
        for (int a = 0; a < 3; ++a) { b.mn[a] = std::fmin(b.mn[a], lo3[a]); b.mx[a] = std::fmax(b.mx[a], hi3[a]); }
    }
    for (int a = 0; a < 3; ++a) { out_lo[a] = b.mn[a]; out_hi[a] = b.mx[a]; }
    out_lo[3] = out_hi[3] = 0.f;
}

// point spacing: median nearest-neighbour distance of a sample of (at most 64 of) the points
inline float point_pitch(const std::vector<TP>& tp) {
    const int m = (int)tp.size(), step = std::max(1, m / 64);
    std::vector<float> nn2;
    for (int i = 0; i < m; i += step) {
        float best = FLT_MAX;
        for (int j = 0; j < m; ++j) {
            const float dx = tp[(size_t)i].x - tp[(size_t)j].x, dy = tp[(size_t)i].y - tp[(size_t)j].y, dz = tp[(size_t)i].z - tp[(size_t)j].z;
            const float d = dx * dx + dy * dy + dz * dz;
            if (d > 0.f && d < best) best = d;
        }
        if (best < FLT_MAX) nn2.push_back(best);
    }
    if (nn2.empty()) return 0.002f;
    std::nth_element(nn2.begin(), nn2.begin() + nn2.size() / 2, nn2.end());
    return std::sqrt(nn2[nn2.size() / 2]);
}

// The uniform grid over the bounding box of the (finite) coordinates: cell edge = cell_factor x the point spacing, enlarged
// until the grid has at most ICP_MAX_CELLS cells.  Sets every point's cell id; ncell stays 0 (sort_by_cell: no table yet).
inline IcpGrid build_grid(std::vector<TP>& tp, float cell_factor) {
    Box bb = box_of_points(tp.data(), tp.data() + tp.size(), true);
    for (int a = 0; a < 3; ++a) if (!(bb.mn[a] <= bb.mx[a])) bb.mn[a] = bb.mx[a] = 0.f;
    float cell = std::fmax(cell_factor * point_pitch(tp), 1.0e-4f);
    int nd[3];
    for (;;) {
        long long tot = 1;
        for (int a = 0; a < 3; ++a) {
            const double cnt = std::floor((double)(bb.mx[a] - bb.mn[a]) / cell) + 1.0;
            nd[a] = cnt > 1.0e6 ? 1000000 : (int)cnt;
            tot *= nd[a];
        }
        if (tot <= ICP_MAX_CELLS) break;
        cell *= 1.26f;
    }
    IcpGrid grid;
    std::memset(&grid, 0, sizeof(grid));
    grid.ox = bb.mn[0]; grid.oy = bb.mn[1]; grid.oz = bb.mn[2];
    grid.cell = cell; grid.inv = 1.0f / cell;
    grid.nx = nd[0]; grid.ny = nd[1]; grid.nz = nd[2];
    auto coord = [&](float v, float o, int n) {
        const float t = std::floor((v - o) * grid.inv);
        return t >= (float)(n - 1) ? n - 1 : (t > 0.f ? (int)t : 0);   // NaN -> 0
    };
    for (TP& t : tp) t.cid = (coord(t.z, grid.oz, grid.nz) * grid.ny + coord(t.y, grid.oy, grid.ny)) * grid.nx + coord(t.x, grid.ox, grid.nx);
    return grid;
}

// Sorts the template by the cells of the grid.  The lane-per-query search of icp_search.hpp scans the few cell rows a query's seed
// ball touches; consecutive runs of 64 stored points are still spatially compact (a strip of one cell row), which is what the
// run boxes of the wave-per-query search feed on.  Each stored point keeps its ORIGINAL index; the nearest-neighbour tie rule
// (lowest original index) is evaluated on that.  Templates the persistent kernels can walk (uint16 positions) also get the
// start table, and the grid its ncell.
inline void sort_by_cell(std::vector<TP>& tp, IcpGrid& grid, std::vector<unsigned short>& cell_start) {
    const int m = (int)tp.size(), ncell = grid.nx * grid.ny * grid.nz;
    std::sort(tp.begin(), tp.end(), [](const TP& a, const TP& bb) { return a.cid < bb.cid || (a.cid == bb.cid && a.oi < bb.oi); });
    if (m > ICP_BIG_MAX) return;
    grid.ncell = ncell;
    cell_start.assign((size_t)ncell + 1, 0);
    int i = 0;
    for (int cid = 0; cid <= ncell; ++cid) {
        while (i < m && tp[(size_t)i].cid < cid) ++i;
        cell_start[(size_t)cid] = (unsigned short)i;
    }
}

// one layout = the points (original index in .w) and the axis-aligned box of every run of 64 consecutive STORED points
// (exact float min/max).  The last run is filled up with points at +inf, original index INT_MAX: kernels that read a whole
// run from global memory - k_icp_pipe_big - meet them as candidates that can never win
inline void run_layout(const std::vector<TP>& tp, int m_pad, std::vector<float4>& pts, std::vector<float4>& lo, std::vector<float4>& hi) {
    const int m = (int)tp.size(), nrun = m_pad / ICP_SUB;
    pts.assign((size_t)m_pad, make_float4(INFINITY, INFINITY, INFINITY, int_bits(0x7fffffff)));
    for (int i = 0; i < m; ++i) pts[(size_t)i] = make_float4(tp[(size_t)i].x, tp[(size_t)i].y, tp[(size_t)i].z, int_bits(tp[(size_t)i].oi));
    lo.resize((size_t)nrun); hi.resize((size_t)nrun);
    for (int r = 0; r < nrun; ++r) {
        const Box b = box_of_points(tp.data() + r * ICP_SUB, tp.data() + std::min(m, (r + 1) * ICP_SUB));
        lo[(size_t)r] = make_float4(b.mn[0], b.mn[1], b.mn[2], 0.f);
        hi[(size_t)r] = make_float4(b.mx[0], b.mx[1], b.mx[2], 0.f);
    }
}

// where a k-d node of n > ICP_SUB points is split: at the median, rounded up so that the left part is a multiple of 64
inline int kd_split_pos(int n) {
    const int k = ((n / 2 + ICP_SUB - 1) / ICP_SUB) * ICP_SUB;
    return k >= n ? k - ICP_SUB : k;
}
inline void record_subtree(Ranges& list, int lo, int hi) {
    bool inside = false;   // already inside a recorded one?
    for (const auto& r : list) inside = inside || (lo >= r.first && hi <= r.second);
    if (!inside) list.push_back({lo, hi});
}
// Layout 2, for the wave-per-query search: compact patches of 64 points from k-d median splits whose left part is a multiple
// of 64, so that consecutive runs of 64 stored points have the smallest boxes the run-box pruning can get.  Of a template that
// does not fit LDS it records the subtrees whose parent is larger than they are: `chunks` of at most ICP_TPL_LDS points and
// `supers` of at most 64 patches (IcpSuper).
inline void kd_patch_order(std::vector<TP>& tp, Ranges& chunks, Ranges& supers) {
    const int m = (int)tp.size();
    Ranges stack = {{0, m}};
    while (!stack.empty()) {
        const auto [lo, hi] = stack.back();
        stack.pop_back();
        const int n = hi - lo;
        if (m > ICP_TPL_LDS && n <= ICP_TPL_LDS) record_subtree(chunks, lo, hi);
        if (m > ICP_TPL_LDS && n <= 64 * ICP_SUB) record_subtree(supers, lo, hi);
        if (n <= ICP_SUB) {
            std::sort(tp.begin() + lo, tp.begin() + hi, [](const TP& a, const TP& bb) { return a.oi < bb.oi; });
            continue;
        }
        const Box b = box_of_points(tp.data() + lo, tp.data() + hi);
        int ax = 0;
        if (b.mx[1] - b.mn[1] > b.mx[ax] - b.mn[ax]) ax = 1;
        if (b.mx[2] - b.mn[2] > b.mx[ax] - b.mn[ax]) ax = 2;
        const int k = kd_split_pos(n);
        auto key = [ax](const TP& t) { return ax == 0 ? t.x : (ax == 1 ? t.y : t.z); };
        std::nth_element(tp.begin() + lo, tp.begin() + lo + k, tp.begin() + hi,
                         [&](const TP& a, const TP& bb) { return key(a) < key(bb) || (key(a) == key(bb) && a.oi < bb.oi); });
        stack.push_back({lo + k, hi});
        stack.push_back({lo, lo + k});
    }
}

// chunk table of a template that does not fit LDS (more than ICP_MAX_CHUNKS subtrees: nchunk stays 0)
inline void fill_chunks(Ranges chunks, int m, const std::vector<float4>& kd_lo, const std::vector<float4>& kd_hi, IcpGrid& grid) {
    if (m <= ICP_TPL_LDS || (int)chunks.size() > ICP_MAX_CHUNKS) return;
    std::sort(chunks.begin(), chunks.end());
    grid.nchunk = (int)chunks.size();
    for (int ci = 0; ci < grid.nchunk; ++ci) {
        const int lo = chunks[(size_t)ci].first, hi = chunks[(size_t)ci].second;
        grid.chunk_start[ci] = lo; grid.chunk_n[ci] = hi - lo;
        box_of_runs(kd_lo, kd_hi, lo / ICP_SUB, (hi + ICP_SUB - 1) / ICP_SUB, grid.chunk_lo[ci], grid.chunk_hi[ci]);
    }
}
// the two halves of the root split (kd_patch_order splits [0, m) at kd_split_pos(m) first; patches are whole on either side)
inline void fill_halves(int m, int m_pad, const std::vector<float4>& kd_lo, const std::vector<float4>& kd_hi, IcpGrid& grid) {
    const int k0 = m > ICP_SUB ? kd_split_pos(m) : m, nrun = m_pad / ICP_SUB;
    grid.kd_split = k0 >= m ? nrun : k0 / ICP_SUB;
    for (int h = 0; h < 2; ++h)   // (an empty half keeps +-FLT_MAX: never reached)
        box_of_runs(kd_lo, kd_hi, h == 0 ? 0 : grid.kd_split, h == 0 ? grid.kd_split : nrun, grid.half_lo[h], grid.half_hi[h]);
}
// The superpatches, and whether k_icp_pipe_big can search the template (returned; su.n = 0 when not): one that does not fit
// LDS and has a cell table, 16-bit positions, at most ICP_BIG_PATCHES patches and at most 64 superpatches that tile them
inline bool fill_supers(Ranges supers, int m, int m_pad, int ncell, const std::vector<float4>& kd_lo, const std::vector<float4>& kd_hi, IcpSuper& su) {
    std::memset(&su, 0, sizeof(su));
    if (m <= ICP_TPL_LDS || m > ICP_BIG_MAX || m_pad / ICP_SUB > ICP_BIG_PATCHES || supers.empty() || supers.size() > 64 || ncell <= 0) return false;
    std::sort(supers.begin(), supers.end());
    su.n = (int)supers.size();
    bool ok = true;
    int covered = 0;   // points tiled so far
    for (int k = 0; k < su.n; ++k) {
        const int lo = supers[(size_t)k].first, hi = supers[(size_t)k].second;
        ok = ok && lo % ICP_SUB == 0 && lo == covered;   // runs of whole patches that tile the template
        covered = hi;
        su.first[k] = lo / ICP_SUB; su.cnt[k] = (hi - lo + ICP_SUB - 1) / ICP_SUB;
        box_of_runs(kd_lo, kd_hi, su.first[k], su.first[k] + su.cnt[k], su.lo[k], su.hi[k]);
    }
    ok = ok && covered == m;
    if (!ok) su.n = 0;
    return ok;
}

// k-d patch r = the cell-sorted positions kdmap[64 r .. 64 r + 63]: the pipelined kernel searches far queries patch by patch
// THROUGH this table (compact boxes) while the points themselves stay cell-sorted in LDS; for a template in global memory
// (k_icp_pipe_big) it turns the position of a k-d ordered point into its cell-sorted one
inline std::vector<unsigned short> kd_to_cell_map(const std::vector<TP>& by_cell, const std::vector<TP>& by_kd, int m_pad) {
    std::vector<int> pos_cell(by_cell.size());   // original index -> position in layout 1
    for (size_t i = 0; i < by_cell.size(); ++i) pos_cell[(size_t)by_cell[i].oi] = (int)i;
    std::vector<unsigned short> kdmap((size_t)m_pad, (unsigned short)std::min(m_pad, 65535));   // padding -> the +inf pad run
    for (size_t i = 0; i < by_kd.size(); ++i) kdmap[i] = (unsigned short)pos_cell[(size_t)by_kd[i].oi];
    return kdmap;
}

}   // namespace tprep

// Pure: the same m packed points and cell_factor (the grid's cell edge in point spacings) give the same bytes.
inline std::shared_ptr<const PreparedTemplate> prepare_template(const float* xyz, int m, float cell_factor) {
    using namespace tprep;
    auto P = std::make_shared<PreparedTemplate>();
    P->m = m;
    P->m_pad = (m + ICP_SUB - 1) / ICP_SUB * ICP_SUB;   // slots start on a 64-point run boundary
    P->xyz.assign(xyz, xyz + 3 * (size_t)m);
    std::vector<TP> tp((size_t)m);
    for (int i = 0; i < m; ++i) tp[(size_t)i] = TP{xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], i, 0};
    P->grid = build_grid(tp, cell_factor);
    sort_by_cell(tp, P->grid, P->cell_start);
    run_layout(tp, P->m_pad, P->cell_pts, P->cell_lo, P->cell_hi);   // layout 1: cell-sorted (whole-cluster kernels)
    const std::vector<TP> by_cell = tp;
    Ranges chunks, supers;
    kd_patch_order(tp, chunks, supers);
    run_layout(tp, P->m_pad, P->kd_pts, P->kd_lo, P->kd_hi);         // layout 2: k-d patches (wave-per-query search)
    fill_chunks(chunks, m, P->kd_lo, P->kd_hi, P->grid);
    fill_halves(m, P->m_pad, P->kd_lo, P->kd_hi, P->grid);
    P->big_ok = fill_supers(supers, m, P->m_pad, P->grid.ncell, P->kd_lo, P->kd_hi, P->super);
    if (m <= ICP_BIG_MAX) P->kdmap = kd_to_cell_map(by_cell, tp, P->m_pad);
    lattice_detect(xyz, m, &P->lat);
    shape_frame_host(xyz, 12, m, &P->frame);
    return P;
}

}   // namespace cd
