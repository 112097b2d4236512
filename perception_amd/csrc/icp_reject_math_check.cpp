// icp_reject_math_check.cpp - host-only run of canonical rule C19's arithmetic through icp_reject_math.hpp
// (tests/test_icp_reject_cpu.py builds and runs it, plain and with sanitizers, and compares what it prints with
// perception_amd/icp_reject.py bit for bit).
//
//   icp_reject_math_check <file>
// <file>: int32 n, int32 bounded, float32 d2_max, int32 0, double factor, then n float32 squared distances, little endian.
// Prints four lines:
//   counts <n> <n0> <kept>
//   median <8 hex digits: the bits of m>          ("median none" with n0 < 3: nothing is selected)
//   thr <16 hex digits: the bits of thr>          ("thr none" likewise)
//   keep <n characters 0 / 1>
// Exit status 2 for a file it cannot read or arguments outside the rule's range.
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_reject_math.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: icp_reject_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[2], zero = 0;
    float d2_max = 0.f;
    double factor = 0.0;
    if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || std::fread(&d2_max, sizeof(float), 1, fp) != 1 || std::fread(&zero, sizeof(int32_t), 1, fp) != 1 ||
        std::fread(&factor, sizeof(double), 1, fp) != 1) { std::fclose(fp); return 2; }
    const int n = head[0], bounded = head[1];
    if (n < 0 || n > (1 << 24) || !(factor > 0.0) || !std::isfinite(factor)) { std::fclose(fp); return 2; }
    std::vector<float> d2((size_t)n);
    if (n > 0 && std::fread(d2.data(), sizeof(float), d2.size(), fp) != d2.size()) { std::fclose(fp); return 2; }
    std::fclose(fp);
    for (float v : d2) if (reject_key(v) > 0x7f800000u) return 2;   // (NaN or signed: not a squared distance of rule C5)

    const float bound = bounded ? d2_max : reject_value(0x7f800000u);
    std::vector<float> k0;
    k0.reserve((size_t)n);
    for (float v : d2) if (icp_in_k0(v, bound)) k0.push_back(v);
    const uint32_t n0 = (uint32_t)k0.size();
    float m = 0.f;
    double thr = 0.0;
    const bool selected = n0 >= (uint32_t)ICP_MIN_CORR;
    if (selected) reject_median_host(k0.data(), n0, factor, &m, &thr);
    std::vector<char> keep((size_t)n);
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        keep[(size_t)i] = icp_in_k0(d2[(size_t)i], bound) && (!selected || reject_keep(d2[(size_t)i], thr));
        kept += keep[(size_t)i];
    }
    std::printf("counts %d %u %d\n", n, n0, kept);
    if (selected) {
        uint64_t tb;
        std::memcpy(&tb, &thr, 8);
        std::printf("median %08x\nthr %016llx\n", reject_key(m), (unsigned long long)tb);
    } else {
        std::printf("median none\nthr none\n");
    }
    std::printf("keep ");
    for (int i = 0; i < n; ++i) std::putchar(keep[(size_t)i] ? '1' : '0');
    std::printf("\n");
    return 0;
}
