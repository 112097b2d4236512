// icp_plane_math_check.cpp - host-only run of canonical rule C17's arithmetic through icp_plane_math.hpp
// (tests/test_icp_plane_cpu.py builds and runs it, plain and with sanitizers, and compares what it prints with
// perception_amd/icp_plane.py bit for bit).
//
//   icp_plane_math_check <file>
// <file>, little endian: int32 mode, int32 count, then count records.
//   mode 0 (solve): a record is int64 sums[28], int32 n, int32 0.  Prints per record
//       T <16 words of 8 hex digits: the bits of T, row-major> <singular>
//   mode 1 (terms): a record is float32 s[3], q[3], lam_it, d2, int32 w, int32 0.  Prints per record
//       t <28 words of 8 hex digits: the bits of the terms>
//     and at the end   sums <28 words of 16 hex digits: rule C4's integer sums over all records>
// Exit status 2 for a file it cannot read.
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_plane_math.hpp"

using namespace cd;

namespace {
struct SolveRec { int64_t sums[PLANE_NSUMS]; int32_t n, pad; };
struct TermRec { float s[3], q[3], lam, d2; int32_t w, pad; };
static_assert(sizeof(SolveRec) == 232 && sizeof(TermRec) == 40, "record layouts of the check file");
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: icp_plane_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[2];
    if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || head[1] < 0 || head[1] > (1 << 22) || (head[0] != 0 && head[0] != 1)) { std::fclose(fp); return 2; }
    const size_t count = (size_t)head[1];
    if (head[0] == 0) {
        std::vector<SolveRec> recs(count);
        if (count > 0 && std::fread(recs.data(), sizeof(SolveRec), count, fp) != count) { std::fclose(fp); return 2; }
        std::fclose(fp);
        for (const SolveRec& r : recs) {
            long long A[PLANE_NSUMS];
            for (int i = 0; i < PLANE_NSUMS; ++i) A[i] = (long long)r.sums[i];
            float T[16];
            const int singular = plane_solve(A, r.n, T);
            std::printf("T");
            for (int i = 0; i < 16; ++i) { uint32_t b; std::memcpy(&b, &T[i], 4); std::printf(" %08x", b); }
            std::printf(" %d\n", singular);
        }
        return 0;
    }
    std::vector<TermRec> recs(count);
    if (count > 0 && std::fread(recs.data(), sizeof(TermRec), count, fp) != count) { std::fclose(fp); return 2; }
    std::fclose(fp);
    unsigned long long sums[PLANE_NSUMS] = {0};
    for (const TermRec& r : recs) {
        const float s[3] = {r.s[0], r.s[1], r.s[2]}, q[3] = {r.q[0], r.q[1], r.q[2]};
        float t[PLANE_NSUMS];
        plane_terms(s, q, r.w, r.lam, r.d2, t);
        std::printf("t");
        for (int i = 0; i < PLANE_NSUMS; ++i) {
            uint32_t b;
            std::memcpy(&b, &t[i], 4);
            std::printf(" %08x", b);
            sums[i] += (unsigned long long)plane_fix(t[i], plane_shift(i));
        }
        std::printf("\n");
    }
    std::printf("sums");
    for (int i = 0; i < PLANE_NSUMS; ++i) std::printf(" %016llx", sums[i]);
    std::printf("\n");
    return 0;
}
