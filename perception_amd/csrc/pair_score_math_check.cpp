// pair_score_math_check.cpp - host-only run of canonical rule C21 through pair_score_math.hpp (tests/test_pair_score_cpu.py builds
// and runs it and compares what it prints with perception_amd/pair_score.py).
//
//   pair_score_math_check <file>
// <file>: int32 m, int32 n, int32 accepted, int32 0, float32 T[16], double max_range, double min_coverage, double
// min_inlier_fraction, then m * 3 float32 (the template, x y z) and n * 3 float32 (the cluster as extracted), little endian.
// Prints two lines:
//   counts <n_source n_source_in n_template n_template_in valid status>
//   values <five words of 16 hex digits: the bits of forward_fitness_in reverse_fitness_in reverse_fitness coverage inlier_fraction>
// Exit status 2 for a file it cannot read or thresholds outside the rule's range.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pair_score_math.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: pair_score_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[4];
    float T[16];
    double lim[3];
    if (std::fread(head, sizeof(int32_t), 4, fp) != 4 || std::fread(T, sizeof(float), 16, fp) != 16 || std::fread(lim, sizeof(double), 3, fp) != 3) { std::fclose(fp); return 2; }
    const int m = head[0], n = head[1];
    if (m < 0 || m > (1 << 24) || n < 0 || n > (1 << 24) || !pair_thresholds_ok(lim[0], lim[1], lim[2])) { std::fclose(fp); return 2; }
    std::vector<float> tpl((size_t)m * 3), src((size_t)n * 3);
    if ((m > 0 && std::fread(tpl.data(), sizeof(float), tpl.size(), fp) != tpl.size()) || (n > 0 && std::fread(src.data(), sizeof(float), src.size(), fp) != src.size())) { std::fclose(fp); return 2; }
    std::fclose(fp);

    const int pre = pair_pre_status(n, m, T);
    unsigned long long acc[PAIR_ACC_PITCH] = {0ull};
    if (pre == CD_OK) pair_passes_host(tpl.data(), m, src.data(), n, T, pair_tau(lim[0]), acc);
    cd_pair_score rec;
    pair_record(n, m, pre, acc, head[2] ? 1 : 0, lim[1], lim[2], &rec);

    std::printf("counts %d %d %d %d %d %d\nvalues", rec.n_source, rec.n_source_in, rec.n_template, rec.n_template_in, rec.valid, rec.status);
    const double v[5] = {rec.forward_fitness_in, rec.reverse_fitness_in, rec.reverse_fitness, rec.coverage, rec.inlier_fraction};
    for (int i = 0; i < 5; ++i) { uint64_t b; std::memcpy(&b, &v[i], 8); std::printf(" %016llx", (unsigned long long)b); }
    std::printf("\n");
    return 0;
}
