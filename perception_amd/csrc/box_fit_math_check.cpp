// box_fit_math_check.cpp - host-only run of canonical rule C24 through box_fit_math.hpp (tests/test_box_fit_cpu.py builds and runs
// it and compares what it prints with perception_amd/box_fit.py).
//
//   box_fit_math_check <file>
// <file>: int32 n_sets, then per set int32 n, int32 have_plane, float32 coeff[4], double band, uint32 loaded_mask, uint32 pad,
// double tolerance, double slot_dims[CD_MAX_TEMPLATES][3], n * 3 float32 (x y z), little endian.
// Prints two lines per set:
//   rec <n n_top hull_vertices edge status overflow match_slot> <23 words of 16 hex digits: the bits of height_ref, dims, pose, area,
//       rectangularity, match_cost>
//   match <slot> <the bits of the cost>       (cd_box_fit_match's rule on the record's dims)
// Exit status 2 for a file it cannot read or arguments outside the rule's range.
#include <cstdio>
#include <cstring>
#include <vector>

#include "box_fit_math.hpp"

using namespace cd;

static void hex(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    std::printf(" %016llx", (unsigned long long)b);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: box_fit_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t n_sets;
    if (std::fread(&n_sets, sizeof(int32_t), 1, fp) != 1 || n_sets < 0 || n_sets > (1 << 20)) { std::fclose(fp); return 2; }
    for (int s = 0; s < n_sets; ++s) {
        int32_t head[2];
        float coeff[4];
        double band, tol, slot_dims[CD_MAX_TEMPLATES][3];
        uint32_t mask[2];
        if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || std::fread(coeff, sizeof(float), 4, fp) != 4 || std::fread(&band, sizeof(double), 1, fp) != 1 ||
            std::fread(mask, sizeof(uint32_t), 2, fp) != 2 || std::fread(&tol, sizeof(double), 1, fp) != 1 ||
            std::fread(slot_dims, sizeof(double), 3 * CD_MAX_TEMPLATES, fp) != 3 * CD_MAX_TEMPLATES) { std::fclose(fp); return 2; }
        const int n = head[0];
        if (n < 0 || n > (1 << 24) || !box_band_ok(band)) { std::fclose(fp); return 2; }
        std::vector<float> xyz((size_t)n * 3);
        if (n > 0 && std::fread(xyz.data(), sizeof(float), xyz.size(), fp) != xyz.size()) { std::fclose(fp); return 2; }
        cd_box_fit r;
        box_fit_host(coeff, xyz.data(), 12, n, band, head[1], &r);
        std::printf("rec %d %d %d %d %d %d %d", r.n, r.n_top, r.hull_vertices, r.edge, r.status, r.overflow, r.match_slot);
        hex(r.height_ref);
        for (int j = 0; j < 3; ++j) hex(r.dims[j]);
        for (int j = 0; j < 16; ++j) hex(r.pose[j]);
        hex(r.area); hex(r.rectangularity); hex(r.match_cost);
        int32_t slot;
        double cost;
        box_match(r.dims, slot_dims, mask[0], tol, &slot, &cost);
        std::printf("\nmatch %d", slot);
        hex(cost);
        std::printf("\n");
    }
    std::fclose(fp);
    return 0;
}
