// prism_math_check.cpp - host-only run of canonical rule C20 through prism_math.hpp (tests/test_table_prism_cpu.py builds and
// runs it and compares what it prints with perception_amd/table_prism.py).
//
//   prism_math_check <file>
// <file>: int32 n_plane, int32 n, float32 coeff[4], double height_min, double height_max, then n_plane * 3 float32 (the plane
// inliers, x y z) and n * 3 float32 (the cloud), little endian.
// Prints four lines:
//   stats <n_before n_kept n_below n_above n_outside hull_vertices axis_u axis_v overflow>
//   hull <hull_vertices pairs u v>
//   height <n words of 16 hex digits: the bits of every point's height>
//   kept <n characters 0 / 1>
// Exit status 2 for a file it cannot read or arguments outside the rule's range.
#include <cstdio>
#include <cstring>
#include <vector>

#include "prism_math.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: prism_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[2];
    float coeff[4];
    double lim[2];
    if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || std::fread(coeff, sizeof(float), 4, fp) != 4 || std::fread(lim, sizeof(double), 2, fp) != 2) { std::fclose(fp); return 2; }
    const int n_plane = head[0], n = head[1];
    if (n_plane < 0 || n_plane > (1 << 24) || n < 0 || n > (1 << 24) || !std::isfinite(lim[0]) || !std::isfinite(lim[1]) || !(lim[0] <= lim[1])) { std::fclose(fp); return 2; }
    std::vector<float> pl((size_t)n_plane * 3), xyz((size_t)n * 3);
    if ((n_plane > 0 && std::fread(pl.data(), sizeof(float), pl.size(), fp) != pl.size()) || (n > 0 && std::fread(xyz.data(), sizeof(float), xyz.size(), fp) != xyz.size())) { std::fclose(fp); return 2; }
    std::fclose(fp);

    // steps 1 - 6
    const PrismPlane P = prism_plane(coeff[0], coeff[1], coeff[2], coeff[3]);
    std::vector<int32_t> puv((size_t)n_plane * 2), hull((size_t)PRISM_MAX_HULL * 2);
    for (int i = 0; i < n_plane; ++i) {
        double h;
        prism_project(P, pl[3 * (size_t)i], pl[3 * (size_t)i + 1], pl[3 * (size_t)i + 2], &h, &puv[2 * (size_t)i], &puv[2 * (size_t)i + 1]);
    }
    PrismRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    int nh = prism_hull_host(puv.data(), n_plane, hull.data(), PRISM_MAX_HULL);
    if (nh > PRISM_MAX_HULL) { rec.overflow = 1; nh = 0; }
    rec.n_before = n; rec.hull_vertices = nh; rec.axis_u = P.k1; rec.axis_v = P.k2;
    // steps 7 and 8
    std::vector<double> height((size_t)n);
    std::vector<char> kept((size_t)n);
    for (int i = 0; i < n; ++i) {
        int32_t u, v;
        prism_project(P, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], &height[(size_t)i], &u, &v);
        const int cls = prism_classify(height[(size_t)i], u, v, lim[0], lim[1], hull.data(), nh);
        kept[(size_t)i] = cls == PRISM_KEPT;
        rec.n_kept += cls == PRISM_KEPT; rec.n_below += cls == PRISM_BELOW; rec.n_above += cls == PRISM_ABOVE; rec.n_outside += cls == PRISM_OUTSIDE;
    }

    std::printf("stats %d %d %d %d %d %d %d %d %d\nhull", rec.n_before, rec.n_kept, rec.n_below, rec.n_above, rec.n_outside, rec.hull_vertices, rec.axis_u,
                rec.axis_v, rec.overflow);
    for (int i = 0; i < 2 * nh; ++i) std::printf(" %d", hull[(size_t)i]);
    std::printf("\nheight");
    for (int i = 0; i < n; ++i) { uint64_t b; std::memcpy(&b, &height[(size_t)i], 8); std::printf(" %016llx", (unsigned long long)b); }
    std::printf("\nkept ");
    for (int i = 0; i < n; ++i) std::putchar(kept[(size_t)i] ? '1' : '0');
    std::printf("\n");
    return 0;
}
