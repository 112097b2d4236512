// template_prep_check.cpp - stand-alone host program (no GPU, no HIP call) around template_prep.hpp.
//   template_prep_check [--check] points.bin        points.bin: raw little-endian float32 xyz triples
// Prepares the template with cell_factor 2 and prints one line of 64-bit FNV-1a digests of everything upload_template sends to
// the device (tests/test_template_prep_cpu.py compares it with the recorded line).  --check also verifies, in plain loops that
// share nothing with the code under test, the invariants the ICP search kernels rely on; the first violation is named, exit 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "template_prep.hpp"

using namespace cd;

static unsigned long long fnv1a(const void* p, size_t n) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
    return h;
}
template <class T> static unsigned long long fnv1a(const std::vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }

static void print_digests(const PreparedTemplate& P) {
    std::printf("m=%d m_pad=%d cell_pts=%016llx cell_lo=%016llx cell_hi=%016llx kd_pts=%016llx kd_lo=%016llx kd_hi=%016llx kdmap=%016llx "
                "cell_start=%016llx grid=%016llx super=%016llx lat=%016llx frame=%016llx big_ok=%d nface=%d frame_status=%d\n",
                P.m, P.m_pad, fnv1a(P.cell_pts), fnv1a(P.cell_lo), fnv1a(P.cell_hi), fnv1a(P.kd_pts), fnv1a(P.kd_lo), fnv1a(P.kd_hi),
                fnv1a(P.kdmap), fnv1a(P.cell_start), fnv1a(&P.grid, sizeof(P.grid)), fnv1a(&P.super, sizeof(P.super)),
                fnv1a(&P.lat, sizeof(P.lat)), fnv1a(&P.frame, sizeof(P.frame)), (int)P.big_ok, P.lat.nface, P.frame.status);
}

// ---- the invariants ---------------------------------------------------------------------------------------------------
static bool violation(const char* fmt, ...) {
    std::va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "template_prep_check: violated: ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
    return false;
}
#define REQUIRE(cond, ...) do { if (!(cond)) return violation(__VA_ARGS__); } while (0)

static int index_of(const float4& p) { int i; std::memcpy(&i, &p.w, 4); return i; }

struct Box3 { float mn[3], mx[3]; };
static const Box3 EMPTY = {{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
static void widen(Box3& b, const float lo[3], const float hi[3]) {
    for (int a = 0; a < 3; ++a) { if (lo[a] < b.mn[a]) b.mn[a] = lo[a]; if (hi[a] > b.mx[a]) b.mx[a] = hi[a]; }
}
static Box3 union_of_runs(const std::vector<float4>& lo, const std::vector<float4>& hi, int r0, int r1) {
    Box3 b = EMPTY;
    for (int r = r0; r < r1; ++r) {
        const float l[3] = {lo[(size_t)r].x, lo[(size_t)r].y, lo[(size_t)r].z}, h[3] = {hi[(size_t)r].x, hi[(size_t)r].y, hi[(size_t)r].z};
        widen(b, l, h);
    }
    return b;
}
static bool same_box(const Box3& b, const float lo[4], const float hi[4]) {
    for (int a = 0; a < 3; ++a) if (!(b.mn[a] == lo[a] && b.mx[a] == hi[a])) return false;
    return lo[3] == 0.f && hi[3] == 0.f;
}

// a layout holds every original point exactly once, then the +inf / INT_MAX pad; every run box is the min/max of its stored points
static bool check_layout(const char* name, const PreparedTemplate& P, const std::vector<float4>& pts, const std::vector<float4>& lo,
                         const std::vector<float4>& hi) {
    const int m = P.m, nrun = P.m_pad / ICP_SUB;
    REQUIRE((int)pts.size() == P.m_pad && (int)lo.size() == nrun && (int)hi.size() == nrun, "%s: array sizes", name);
    std::vector<char> seen((size_t)m, 0);
    for (int i = 0; i < m; ++i) {
        const int oi = index_of(pts[(size_t)i]);
        REQUIRE(oi >= 0 && oi < m, "%s: position %d holds index %d outside 0..m-1", name, i, oi);
        REQUIRE(!seen[(size_t)oi], "%s: original index %d stored twice (second at position %d)", name, oi, i);
        seen[(size_t)oi] = 1;
        REQUIRE(std::memcmp(&pts[(size_t)i], &P.xyz[3 * (size_t)oi], 12) == 0, "%s: position %d is not the caller's point %d", name, i, oi);
    }
    for (int i = m; i < P.m_pad; ++i) {
        const float4 p = pts[(size_t)i];
        REQUIRE(p.x == INFINITY && p.y == INFINITY && p.z == INFINITY && index_of(p) == 0x7fffffff, "%s: pad position %d is not (+inf, INT_MAX)", name, i);
    }
    for (int r = 0; r < nrun; ++r) {
        Box3 b = EMPTY;
        for (int i = r * ICP_SUB; i < m && i < (r + 1) * ICP_SUB; ++i) {
            const float v[3] = {pts[(size_t)i].x, pts[(size_t)i].y, pts[(size_t)i].z};
            widen(b, v, v);
        }
        const float l[4] = {lo[(size_t)r].x, lo[(size_t)r].y, lo[(size_t)r].z, lo[(size_t)r].w}, h[4] = {hi[(size_t)r].x, hi[(size_t)r].y, hi[(size_t)r].z, hi[(size_t)r].w};
        REQUIRE(same_box(b, l, h), "%s: box of run %d is not the min/max of its stored points", name, r);
    }
    return true;
}

// IcpGrid's documented formula (common.hpp): clamp((int)floorf((v - o) * inv), 0, n - 1), compared as floats so that no cast overflows
static int cell_coord(float v, float o, float inv, int n) {
    const float t = std::floor((v - o) * inv);
    if (t >= (float)(n - 1)) return n - 1;
    return t > 0.f ? (int)t : 0;
}

static bool check_cells(const PreparedTemplate& P) {
    const IcpGrid& g = P.grid;
    const int m = P.m;
    REQUIRE(g.nx >= 1 && g.ny >= 1 && g.nz >= 1 && (long long)g.nx * g.ny * g.nz <= ICP_MAX_CELLS, "grid: %d x %d x %d cells", g.nx, g.ny, g.nz);
    const int ncell = g.nx * g.ny * g.nz;
    std::vector<int> cid((size_t)m), count((size_t)ncell + 1, 0);
    for (int i = 0; i < m; ++i) {
        const float4 p = P.cell_pts[(size_t)i];
        cid[(size_t)i] = (cell_coord(p.z, g.oz, g.inv, g.nz) * g.ny + cell_coord(p.y, g.oy, g.inv, g.ny)) * g.nx + cell_coord(p.x, g.ox, g.inv, g.nx);
        ++count[(size_t)cid[(size_t)i]];
        if (i == 0) continue;
        const bool ordered = cid[(size_t)i - 1] < cid[(size_t)i] ||
                             (cid[(size_t)i - 1] == cid[(size_t)i] && index_of(P.cell_pts[(size_t)i - 1]) < index_of(p));
        REQUIRE(ordered, "cell_pts: positions %d and %d are not in (cell, original index) order", i - 1, i);
    }
    if (m > ICP_BIG_MAX) {
        REQUIRE(g.ncell == 0 && P.cell_start.empty() && P.kdmap.empty(), "a template above ICP_BIG_MAX has a cell table or a kdmap");
        return true;
    }
    REQUIRE(g.ncell == ncell && (int)P.cell_start.size() == ncell + 1, "cell_start: %d entries for %d cells (grid.ncell = %d)", (int)P.cell_start.size(), ncell, g.ncell);
    int below = 0;   // stored points with a cell id < c
    for (int c = 0; c <= ncell; ++c) {
        REQUIRE((int)P.cell_start[(size_t)c] == below, "cell_start[%d] = %d, but %d stored points have a smaller cell id", c, (int)P.cell_start[(size_t)c], below);
        below += count[(size_t)c];
    }
    return true;
}

static bool check_kd(const PreparedTemplate& P) {
    const int m = P.m, m_pad = P.m_pad, nrun = m_pad / ICP_SUB;
    for (int i = 1; i < m; ++i)
        REQUIRE(i % ICP_SUB == 0 || index_of(P.kd_pts[(size_t)i - 1]) < index_of(P.kd_pts[(size_t)i]), "kd_pts: patch %d is not in ascending original index at position %d", i / ICP_SUB, i);
    if (m <= ICP_BIG_MAX) {
        REQUIRE((int)P.kdmap.size() == m_pad, "kdmap: %d entries, m_pad = %d", (int)P.kdmap.size(), m_pad);
        std::vector<int> pos_cell((size_t)m);
        for (int i = 0; i < m; ++i) pos_cell[(size_t)index_of(P.cell_pts[(size_t)i])] = i;
        for (int i = 0; i < m; ++i)
            REQUIRE((int)P.kdmap[(size_t)i] == pos_cell[(size_t)index_of(P.kd_pts[(size_t)i])], "kdmap[%d] = %d is not the cell-sorted position of that point", i, (int)P.kdmap[(size_t)i]);
        for (int i = m; i < m_pad; ++i)
            REQUIRE((int)P.kdmap[(size_t)i] == (m_pad < 65535 ? m_pad : 65535), "kdmap[%d] = %d: a pad does not map to min(m_pad, 65535)", i, (int)P.kdmap[(size_t)i]);
    }
    const IcpGrid& g = P.grid;
    REQUIRE(g.nchunk >= 0 && g.nchunk <= ICP_MAX_CHUNKS && (m > ICP_TPL_LDS || g.nchunk == 0), "nchunk = %d", g.nchunk);
    int covered = 0;
    for (int c = 0; c < g.nchunk; ++c) {
        const int lo = g.chunk_start[c], n = g.chunk_n[c];
        REQUIRE(lo == covered && lo % ICP_SUB == 0, "chunk %d starts at %d: not where chunk %d ends (%d), or not on a multiple of 64", c, lo, c - 1, covered);
        REQUIRE(n >= 1 && n <= ICP_TPL_LDS, "chunk %d holds %d points", c, n);
        covered = lo + n;
        REQUIRE(covered <= m, "chunk %d ends at %d, beyond m", c, covered);
        REQUIRE(same_box(union_of_runs(P.kd_lo, P.kd_hi, lo / ICP_SUB, (covered + ICP_SUB - 1) / ICP_SUB), g.chunk_lo[c], g.chunk_hi[c]), "chunk %d: box is not the union of its run boxes", c);
    }
    REQUIRE(g.nchunk == 0 || covered == m, "the chunks cover [0, %d), not [0, m)", covered);
    int split = nrun;   // the root split: the median rounded up to whole patches; a template of one patch has no right half
    if (m > ICP_SUB) {
        int k = (m / 2 + ICP_SUB - 1) / ICP_SUB * ICP_SUB;
        if (k >= m) k -= ICP_SUB;
        split = k / ICP_SUB;
    }
    REQUIRE(g.kd_split == split, "kd_split = %d, the root split is at patch %d", g.kd_split, split);
    for (int h = 0; h < 2; ++h)
        REQUIRE(same_box(union_of_runs(P.kd_lo, P.kd_hi, h == 0 ? 0 : split, h == 0 ? split : nrun), g.half_lo[h], g.half_hi[h]), "half %d: box is not the union of its run boxes", h);
    const IcpSuper& s = P.super;
    if (!P.big_ok) {
        REQUIRE(s.n == 0, "big_ok is off but super.n = %d", s.n);
        return true;
    }
    REQUIRE(m > ICP_TPL_LDS && m <= ICP_BIG_MAX && nrun <= ICP_BIG_PATCHES && g.ncell > 0 && s.n >= 1 && s.n <= 64, "big_ok for m = %d, ncell = %d, super.n = %d", m, g.ncell, s.n);
    int next = 0;
    for (int k = 0; k < s.n; ++k) {
        REQUIRE(s.first[k] == next && s.cnt[k] >= 1 && s.cnt[k] <= 64, "superpatch %d: first = %d, cnt = %d after patch %d", k, s.first[k], s.cnt[k], next);
        next += s.cnt[k];
        REQUIRE(next <= nrun, "superpatch %d ends beyond the last patch", k);
        REQUIRE(same_box(union_of_runs(P.kd_lo, P.kd_hi, s.first[k], next), s.lo[k], s.hi[k]), "superpatch %d: box is not the union of its patches' boxes", k);
    }
    REQUIRE(next == nrun, "the superpatches tile %d of %d patches", next, nrun);
    return true;
}

int main(int argc, char** argv) {
    const bool check = argc == 3 && std::string(argv[1]) == "--check";
    if (argc != (check ? 3 : 2)) { std::fprintf(stderr, "usage: template_prep_check [--check] points.bin\n"); return 2; }
    std::FILE* f = std::fopen(argv[argc - 1], "rb");
    if (!f) { std::fprintf(stderr, "template_prep_check: cannot open %s\n", argv[argc - 1]); return 2; }
    std::vector<float> xyz;
    float buf[3 * 1024];
    size_t got;
    while ((got = std::fread(buf, 4, 3 * 1024, f)) > 0) xyz.insert(xyz.end(), buf, buf + got);
    std::fclose(f);
    if (xyz.empty() || xyz.size() % 3 != 0) { std::fprintf(stderr, "template_prep_check: %s does not hold xyz triples\n", argv[argc - 1]); return 2; }
    const std::shared_ptr<const PreparedTemplate> P = prepare_template(xyz.data(), (int)(xyz.size() / 3), 2.0f);
    print_digests(*P);
    if (!check) return 0;
    if (P->m_pad != (P->m + ICP_SUB - 1) / ICP_SUB * ICP_SUB) return violation("m_pad = %d for m = %d", P->m_pad, P->m), 1;
    const bool ok = check_layout("cell_pts", *P, P->cell_pts, P->cell_lo, P->cell_hi) && check_layout("kd_pts", *P, P->kd_pts, P->kd_lo, P->kd_hi) &&
                    check_cells(*P) && check_kd(*P);
    return ok ? 0 : 1;
}
