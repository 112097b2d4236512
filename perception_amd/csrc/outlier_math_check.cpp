// outlier_math_check.cpp - host-only run of canonical rule C16 through outlier_math.hpp (tests/test_outlier_filter_cpu.py builds
// and runs it, plain and with sanitizers, and compares what it prints with perception_amd/outlier_filter.py).
//
//   outlier_math_check <file>
// <file>: int32 n, int32 mean_k, int32 negative, int32 0, double std_mul, then n * 3 float32 (x y z), little endian.
// Prints four lines:
//   counts <n> <m> <computed> <kept>
//   dist <n words of 8 hex digits: the bits of every dist_i, 0 for a dropped point>
//   stats <3 words of 16 hex digits: the bits of mean, stddev, threshold>
//   kept <n characters 0 / 1>
// Exit status 2 for a file it cannot read or arguments outside the rule's range.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "outlier_math.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: outlier_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[4];
    double std_mul = 0.0;
    if (std::fread(head, sizeof(int32_t), 4, fp) != 4 || std::fread(&std_mul, sizeof(double), 1, fp) != 1) { std::fclose(fp); return 2; }
    const int n = head[0], mean_k = head[1], negative = head[2];
    if (n < 0 || n > (1 << 24) || mean_k < 1 || mean_k > OUTLIER_MAX_K || !std::isfinite(std_mul)) { std::fclose(fp); return 2; }
    std::vector<float> xyz((size_t)n * 3);
    if (n > 0 && std::fread(xyz.data(), sizeof(float), xyz.size(), fp) != xyz.size()) { std::fclose(fp); return 2; }
    std::fclose(fp);

    // step 1
    std::vector<char> fin((size_t)n);
    int m = 0;
    for (int i = 0; i < n; ++i) { fin[(size_t)i] = outlier_finite(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]); m += fin[(size_t)i]; }
    // steps 3 and 4: every finite candidate's key, the mean_k + 1 smallest in ascending order
    std::vector<float> dist((size_t)n, 0.0f);
    std::vector<uint32_t> keys;
    keys.reserve((size_t)m + (size_t)mean_k + 1);
    for (int i = 0; i < n; ++i) {
        if (!fin[(size_t)i]) continue;
        keys.clear();
        const float* q = &xyz[3 * (size_t)i];
        for (int j = 0; j < n; ++j)
            if (fin[(size_t)j]) keys.push_back(outlier_d2_key(q[0], q[1], q[2], xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2]));
        while ((int)keys.size() < mean_k + 1) keys.push_back(OUTLIER_NO_KEY);
        std::partial_sort(keys.begin(), keys.begin() + mean_k + 1, keys.end());
        if (keys[(size_t)mean_k] != OUTLIER_NO_KEY)   // (else step 2: no more than mean_k finite points, dist stays 0)
            dist[(size_t)i] = outlier_mean_dist([&](int k) { return outlier_root(keys[(size_t)k]); }, mean_k);
    }
    // steps 2, 5 and 6
    OutlierRecord rec;
    std::memset(&rec, 0, sizeof(rec));
    rec.n_before = n; rec.n_finite = m; rec.computed = m > mean_k;
    if (rec.computed) {
        OutlierSums s = {0.0, 0.0};
        for (int i = 0; i < n; ++i) outlier_accumulate(s, dist[(size_t)i]);
        outlier_statistics(s, m, std_mul, &rec);
    }
    std::vector<char> kept((size_t)n);
    for (int i = 0; i < n; ++i) {
        kept[(size_t)i] = fin[(size_t)i] && (!rec.computed || outlier_keep(dist[(size_t)i], rec.threshold, negative));
        rec.n_kept += kept[(size_t)i];
    }

    std::printf("counts %d %d %d %d\ndist", n, m, rec.computed, rec.n_kept);
    for (int i = 0; i < n; ++i) { uint32_t b; std::memcpy(&b, &dist[(size_t)i], 4); std::printf(" %08x", b); }
    std::printf("\nstats");
    for (double v : {rec.mean, rec.stddev, rec.threshold}) { uint64_t b; std::memcpy(&b, &v, 8); std::printf(" %016llx", (unsigned long long)b); }
    std::printf("\nkept ");
    for (int i = 0; i < n; ++i) std::putchar(kept[(size_t)i] ? '1' : '0');
    std::printf("\n");
    return 0;
}
