// icp_recip_math_check.cpp - host-only run of canonical rule C22's arithmetic through icp_recip_math.hpp
// (tests/test_icp_recip_cpu.py builds and runs it, plain and with sanitizers, and compares what it prints with
// perception_amd/icp_reciprocal.py bit for bit).
//
//   icp_recip_math_check <file>
// <file>: int32 n, int32 m, int32 bounded, float32 d2_max, then n source points and m template points (x, y, z float32), little
// endian.  The correspondences are rule C5's by brute force (ties to the lowest template index).  Prints four lines:
//   counts <n> <n0> <kept>
//   nn <n indices>
//   d2 <n times 8 hex digits: the bits of d2>
//   keep <n characters 0 / 1>
// Exit status 2 for a file it cannot read or sizes outside 1 .. 2^20.
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_recip_math.hpp"

using namespace cd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: icp_recip_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[3];
    float d2_max = 0.f;
    if (std::fread(head, sizeof(int32_t), 3, fp) != 3 || std::fread(&d2_max, sizeof(float), 1, fp) != 1) { std::fclose(fp); return 2; }
    const int n = head[0], m = head[1], bounded = head[2];
    if (n < 1 || n > (1 << 20) || m < 1 || m > (1 << 20)) { std::fclose(fp); return 2; }
    std::vector<float> src(3 * (size_t)n), tpl(3 * (size_t)m);
    if (std::fread(src.data(), sizeof(float), src.size(), fp) != src.size() || std::fread(tpl.data(), sizeof(float), tpl.size(), fp) != tpl.size()) {
        std::fclose(fp);
        return 2;
    }
    std::fclose(fp);

    std::vector<int32_t> nn((size_t)n);
    std::vector<float> d2((size_t)n);
    for (int i = 0; i < n; ++i) nn[(size_t)i] = recip_forward_host(tpl.data(), 3, m, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], &d2[(size_t)i]);
    std::vector<uint8_t> keep((size_t)n);
    const int n0 = recip_mask_host(src.data(), 3, n, tpl.data(), 3, bounded ? d2_max : std::numeric_limits<float>::infinity(), nn.data(), d2.data(), keep.data());
    int kept = 0;
    for (int i = 0; i < n; ++i) kept += keep[(size_t)i];
    std::printf("counts %d %d %d\nnn", n, n0, kept);
    for (int i = 0; i < n; ++i) std::printf(" %d", nn[(size_t)i]);
    std::printf("\nd2 ");
    for (int i = 0; i < n; ++i) {
        uint32_t b;
        std::memcpy(&b, &d2[(size_t)i], 4);
        std::printf("%08x", b);
    }
    std::printf("\nkeep ");
    for (int i = 0; i < n; ++i) std::putchar(keep[(size_t)i] ? '1' : '0');
    std::printf("\n");
    return 0;
}
