// label_math_check.cpp - host-only check of label_math.hpp (tests/test_point_labels_cpu.py builds and runs it; see the Makefile for
// a sanitizer build).  For a few hundred deterministic grids - a leaf, a crop, a cloud of kept points that defines the grid's
// min_b / div_b and the occupied cells, a class per cell - it labels probe points (points of the cloud, points on cell
// boundaries, points in empty cells, points far outside the grid, NaN and +-inf) twice: with the key arithmetic and the binary
// search of label_math.hpp (the single search and the four-in-step form the kernel runs) in BOTH key forms (PCL's idx, the packed
// bit fields), and with a plain loop that keeps the cell
// coordinates in double / int64 and looks the cell up by walking the list of occupied cells.  Every label must agree.
//
//   label_math_check [grids]      prints "ok <grids> <probes> <hits> <outside>", exit status 1 on a difference
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "label_math.hpp"

using namespace cd;

static uint64_t g_state = 20190409ull;
static uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * (1.0 / 9007199254740992.0)); }

struct Cell { long long i, j, k; };
static bool cell_less(const Cell& a, const Cell& b) { return a.k != b.k ? a.k < b.k : (a.j != b.j ? a.j < b.j : a.i < b.i); }
static bool cell_same(const Cell& a, const Cell& b) { return a.i == b.i && a.j == b.j && a.k == b.k; }

// the cell of a finite point, the product in float32 as the rule has it, everything after it in double / int64
static bool plain_cell(const float p[3], float inv, Cell* c) {
    double f[3];
    for (int a = 0; a < 3; ++a) {
        const float prod = p[a] * inv;
        f[a] = std::floor((double)prod);
        if (!(std::fabs(f[a]) < 4.0e18)) return false;
    }
    c->i = (long long)f[0]; c->j = (long long)f[1]; c->k = (long long)f[2];
    return true;
}

int main(int argc, char** argv) {
    const int grids = argc > 1 ? std::atoi(argv[1]) : 300;
    long long n_probes = 0, n_hits = 0, n_outside = 0;
    for (int gi = 0; gi < grids; ++gi) {
        const float leafs[4] = {0.005f, 0.001f, 0.01f, 0.0173f};
        const float leaf = leafs[gi & 3], inv = 1.0f / leaf;
        CropLimits lim = {0.0f, 0.9f, -0.2f, 0.2f};
        if (gi % 5 == 4) { lim.zlo = 0.25f; lim.zhi = 0.5f; lim.xlo = -0.05f; lim.xhi = 0.15f; }
        // ---- the cloud: a slanted sheet and a blob, some points exactly on cell boundaries
        std::vector<float> pts;
        const int n = 200 + (int)(next_u64() % 1800);
        const double ylo = uni(-0.4, 0.0), yhi = ylo + uni(0.05, 0.6);
        for (int q = 0; q < n; ++q) {
            float p[3] = {(float)uni(lim.xlo, lim.xhi), (float)uni(ylo, yhi), (float)uni(lim.zlo, lim.zhi)};
            if (q % 7 == 0) p[q % 3] = (float)((double)(long long)(p[q % 3] * inv)) * leaf;   // a multiple of the leaf, or next to one
            if (q % 11 == 0) p[2] = (float)(0.3 + 0.2 * p[0]);
            if (!label_finite(p[0], p[1], p[2]) || !label_kept(p[0], p[2], lim)) continue;
            pts.insert(pts.end(), p, p + 3);
        }
        const int m = (int)pts.size() / 3;
        if (m == 0) continue;
        // ---- the grid (k_voxel_setup) and the occupied cells in idx order, each with a class
        std::vector<Cell> cells((size_t)m);
        Cell mn = {0, 0, 0}, mx = {0, 0, 0};
        for (int q = 0; q < m; ++q) {
            if (!plain_cell(&pts[3 * (size_t)q], inv, &cells[(size_t)q])) { std::fprintf(stderr, "grid %d: a kept point has no cell\n", gi); return 1; }
            const Cell& c = cells[(size_t)q];
            if (q == 0) mn = mx = c;
            mn.i = std::min(mn.i, c.i); mn.j = std::min(mn.j, c.j); mn.k = std::min(mn.k, c.k);
            mx.i = std::max(mx.i, c.i); mx.j = std::max(mx.j, c.j); mx.k = std::max(mx.k, c.k);
        }
        std::vector<Cell> occ(cells);
        std::sort(occ.begin(), occ.end(), cell_less);
        occ.erase(std::unique(occ.begin(), occ.end(), cell_same), occ.end());
        const int nv = (int)occ.size();
        LabelGrid g;
        g.min_b[0] = (int)mn.i; g.min_b[1] = (int)mn.j; g.min_b[2] = (int)mn.k;
        g.div_b[0] = (int)(mx.i - mn.i + 1); g.div_b[1] = (int)(mx.j - mn.j + 1); g.div_b[2] = (int)(mx.k - mn.k + 1);
        // the packed form: fields from the crop limits as stage_crop_voxel sizes them
        KeyPack kp;
        {
            const float fl[4] = {std::floor(lim.xlo * inv), std::floor(lim.xhi * inv), std::floor(lim.zlo * inv), std::floor(lim.zhi * inv)};
            const long long ri = (long long)fl[1] - (long long)fl[0] + 1, rk = (long long)fl[3] - (long long)fl[2] + 1;
            int bi = 1, bk = 1;
            while ((1ll << bi) < ri) ++bi;
            while ((1ll << bk) < rk) ++bk;
            if (bi + bk > 20) { std::fprintf(stderr, "grid %d: the crop does not bound the fields\n", gi); return 1; }
            kp.enabled = 1; kp.bi = bi; kp.bj = 32 - bi - bk;
            kp.ilo = (int)fl[0]; kp.klo = (int)fl[2]; kp.jlo = -(1 << (kp.bj - 1));
            if (kp.bj >= 11) kp.jlo -= 256;
        }
        std::vector<uint32_t> key_idx((size_t)nv), key_packed((size_t)nv);
        std::vector<uint8_t> cls((size_t)nv);
        for (int v = 0; v < nv; ++v) {
            const Cell& c = occ[(size_t)v];
            key_idx[(size_t)v] = (uint32_t)((c.i - mn.i) + (c.j - mn.j) * g.div_b[0] + (c.k - mn.k) * (long long)g.div_b[0] * g.div_b[1]);
            key_packed[(size_t)v] = (uint32_t)(c.i - kp.ilo) | ((uint32_t)(c.j - kp.jlo) << kp.bi) | ((uint32_t)(c.k - kp.klo) << (kp.bi + kp.bj));
            const int r = (int)(next_u64() % 300) - 10;   // a cluster label: -10 .. 289
            const uint64_t kind = next_u64() % 4;
            cls[(size_t)v] = kind == 0 ? (uint8_t)LABEL_PLANE : (kind == 1 ? (uint8_t)LABEL_GATED : label_of_rank(r));
            const uint8_t want = (r >= 0 && r < 248) ? (uint8_t)(8 + r) : (uint8_t)3;
            if (kind >= 2 && cls[(size_t)v] != want) { std::fprintf(stderr, "label_of_rank(%d) = %d\n", r, (int)cls[(size_t)v]); return 1; }
        }
        for (int v = 1; v < nv; ++v)
            if (!(key_idx[(size_t)v - 1] < key_idx[(size_t)v]) || !(key_packed[(size_t)v - 1] < key_packed[(size_t)v])) {
                std::fprintf(stderr, "grid %d: the keys of the occupied cells are not ascending in both forms\n", gi);
                return 1;
            }
        // ---- probes
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const int probes = 3 * m + 64;
        for (int q = 0; q < probes; ++q) {
            float p[3];
            const int kind = q < m ? 0 : (int)(next_u64() % 8) + 1;
            if (kind == 0) std::memcpy(p, &pts[3 * (size_t)q], 12);                                     // the call's own points
            else {
                const float* src = &pts[3 * (size_t)(next_u64() % (uint64_t)m)];
                std::memcpy(p, src, 12);
                if (kind == 1) p[next_u64() % 3] += leaf * (float)((int)(next_u64() % 9) - 4);             // a neighbouring cell, perhaps empty
                if (kind == 2) { const int a = (int)(next_u64() % 3); p[a] = (float)std::floor((double)(p[a] * inv)) * leaf; }   // on a boundary
                if (kind == 3) p[1] = (float)uni(-5.0e3, 5.0e3);                                         // y outside the grid, mostly outside its bit field
                if (kind == 4) { p[0] = (float)uni(-1.0, 1.0); p[2] = (float)uni(-0.5, 2.0); }          // across the crop limits
                if (kind == 5) p[next_u64() % 3] = (next_u64() & 1) ? inf : -inf;
                if (kind == 6) p[next_u64() % 3] = nan;
                if (kind == 7) p[1] = (float)uni(-3.0e38, 3.0e38);                                       // finite, the product overflows
                if (kind == 8) p[1] = (float)uni(-1.0e7, 1.0e7);                                         // beyond int32 cells at the small leaves
            }
            ++n_probes;
            // plain
            uint8_t want = (uint8_t)LABEL_INVALID;
            const bool fin = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
            if (fin) {
                const bool kept = !((double)p[2] < (double)lim.zlo) && !((double)p[2] > (double)lim.zhi) && !((double)p[0] < (double)lim.xlo) && !((double)p[0] > (double)lim.xhi);
                want = (uint8_t)LABEL_CROPPED;
                if (kept) {
                    want = (uint8_t)LABEL_GATED;
                    Cell c;
                    bool found = false;
                    if (plain_cell(p, inv, &c))
                        for (int v = 0; v < nv && !found; ++v)
                            if (cell_same(occ[(size_t)v], c)) { want = cls[(size_t)v]; found = true; }
                    n_hits += found;
                    n_outside += !found;
                }
            }
            // label_math.hpp, both key forms
            for (int form = 0; form < 2; ++form) {
                uint8_t got = (uint8_t)LABEL_INVALID;
                if (label_finite(p[0], p[1], p[2])) {
                    got = (uint8_t)LABEL_CROPPED;
                    if (label_kept(p[0], p[2], lim)) {
                        got = (uint8_t)LABEL_GATED;
                        uint32_t key = 0;
                        const bool in = form ? label_key_packed(p[0], p[1], p[2], inv, kp, &key) : label_key_idx(p[0], p[1], p[2], inv, g, &key);
                        if (in) {
                            const std::vector<uint32_t>& keys = form ? key_packed : key_idx;
                            const int at = label_lower_bound(keys.data(), nv, key);
                            if (at < 0 || at > nv) { std::fprintf(stderr, "grid %d: lower bound %d outside 0 .. %d\n", gi, at, nv); return 1; }
                            // the in-step search of the kernel: this key beside three others, one of them in a finished (n = 0) search
                            const uint32_t* const tabs[4] = {key_idx.data(), keys.data(), key_packed.data(), keys.data()};
                            const int ns[4] = {nv, nv, 0, nv > 1 ? nv - 1 : 1};
                            const uint32_t ks[4] = {(uint32_t)next_u64(), key, key, key ^ 1u};
                            int ats[4];
                            label_lower_bound_n<4>(tabs, ns, ks, ats);
                            if (ats[1] != at || ats[2] != 0 || ats[0] != label_lower_bound(tabs[0], ns[0], ks[0]) || ats[3] != label_lower_bound(tabs[3], ns[3], ks[3])) {
                                std::fprintf(stderr, "grid %d probe %d: the in-step search differs from the single one\n", gi, q);
                                return 1;
                            }
                            if (at < nv && keys[(size_t)at] == key) got = cls[(size_t)at];
                        }
                    }
                }
                if (got != want) {
                    std::fprintf(stderr, "grid %d probe %d (kind %d, %s keys): point %.9g %.9g %.9g label %d, the plain loop says %d\n", gi, q, kind,
                                 form ? "packed" : "idx", (double)p[0], (double)p[1], (double)p[2], (int)got, (int)want);
                    return 1;
                }
            }
        }
    }
    // the tint of one channel against its definition, every (c, p, a)
    for (uint32_t a = 0; a < 256; ++a)
        for (uint32_t c = 0; c < 256; c += 5)
            for (uint32_t p = 0; p < 256; p += 3) {
                const double exact = std::floor(((double)c * (255.0 - a) + (double)p * a + 127.0) / 255.0);
                if ((double)label_tint(c, p, a) != exact) { std::fprintf(stderr, "tint(%u, %u, %u)\n", c, p, a); return 1; }
            }
    std::printf("ok %d %lld %lld %lld\n", grids, n_probes, n_hits, n_outside);
    return 0;
}
