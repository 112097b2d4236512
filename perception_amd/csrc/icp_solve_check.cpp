// icp_solve_check.cpp - host-only runner of icp_step (icp_solve.hpp), the single-lane ICP iteration update every driver calls,
// compiled from the header the device uses with -ffp-contract=off.  It keeps NO reference of its own: it reads records, runs
// icp_step<false> or icp_step<true> on each and writes the outgoing states; tests/test_icp_solve_truth_cpu.py holds what comes
// out against a float64 Umeyama written from the definition (tests/icp_solve_reference.py).  See the Makefile for a sanitizer build.
//
//   icp_solve_check <in> <out>
//   in:  int64 k, int64 bounded, int64 max_iter, double trans_eps, rel_mse, rot_thr, abs_mse;
//        uint64 sums[k][16]; int32 n[k]; IcpState in[k]
//   out: IcpState out[k]; int32 done[k]
//   exit status 2 on a malformed file
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
namespace cd {   // device-only helpers that icp_solve.hpp names in a template this program never instantiates
long long fixq(float v, int shift);
unsigned long long fixq_fast(float v, int shift);
}
float __fmul_rn(float a, float b);
#include "icp_solve.hpp"

using namespace cd;

static_assert(sizeof(IcpState) == 152, "the record layout of the files (capi.ICP_STATE)");

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: icp_solve_check <in> <out>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    long long head[3];
    double crit[4];
    if (std::fread(head, 8, 3, f) != 3 || std::fread(crit, 8, 4, f) != 4 || head[0] < 0 || head[0] > (1ll << 24)) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t k = (size_t)head[0];
    const bool bounded = head[1] != 0;
    IcpParams prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.max_iter = (int32_t)head[2];
    prm.trans_eps = crit[0]; prm.rel_mse = crit[1]; prm.rot_thr = crit[2]; prm.abs_mse = crit[3];
    std::vector<unsigned long long> sums;
    std::vector<int32_t> n;
    std::vector<IcpState> st;
    if (!read_n(f, sums, 16 * k) || !read_n(f, n, k) || !read_n(f, st, k) || std::fgetc(f) != EOF) {
        std::fprintf(stderr, "bad length for %zu records\n", k);
        return 2;
    }
    std::fclose(f);
    std::vector<int32_t> done(k);
    for (size_t i = 0; i < k; ++i)
        done[i] = bounded ? icp_step<true>(st[i], &sums[16 * i], n[i], prm) : icp_step<false>(st[i], &sums[16 * i], n[i], prm);
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = (k == 0 || (std::fwrite(st.data(), sizeof(IcpState), k, f) == k && std::fwrite(done.data(), 4, k, f) == k));
    if (std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
