// icp_solve_row_check.cpp - host-only proof that icp_step_row (icp_solve_row.hpp) computes what icp_step (icp_solve.hpp) does
// (tests/test_icp_solve_row_cpu.py builds and runs it; see the Makefile for a sanitizer build).  The row is emulated by arrays
// of 16 lanes: each() is a loop over the lanes, read() an array access.  Both functions are compiled from the headers the device
// uses, with -ffp-contract=off; on the host sqrt_ge1 / rcp_ge1 are std::sqrt and 1.0f / x inside their domains (their device forms
// are checked exhaustively on the device, cd_icp_solve_batch) and a wrong value outside, so that a rotation which keeps the short
// form with an argument out of range is found here.  Every byte of the outgoing IcpState and the return value must agree on
//   * random moment sets (default 1e7): dense, scaled by 1e-9 .. 1e3, symmetric, sparse, equal singular values, rank 2 with
//     either sign of det U * det V, moments of real point pairs; random incoming states and parameter sets;
//   * structured ones: zero covariance, rank 1 and 2, det(sigma) < 0, m00 + m11 == 0, an exactly zero off-diagonal (y == 0 in
//     make_jacobi), diagonal matrices, sums at +-2^62 and of one unit, n = 0 (the means become inf and NaN and flow through every
//     operation; the sums themselves are integers and cannot be NaN), n = 0 .. 3 with BOUNDED;
//   * every convergence branch (counted, each must occur): BOUNDED stop, iteration limit, rotation / translation epsilon,
//     absolute MSE, relative MSE, not converged.
//
//   icp_solve_row_check [random sets]   prints "ok <sets> <stop> <limit> <eps> <abs> <rel> <open> <rank2>", exit status 1 on a difference
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "common.hpp"
namespace cd {   // device-only helpers that icp_solve.hpp names in a template this program never instantiates
long long fixq(float v, int shift);
unsigned long long fixq_fast(float v, int shift);
}
float __fmul_rn(float a, float b);
#define CD_ROW_POISON 1   // sqrt_ge1 / rcp_ge1 answer 12345 outside their domains: row_rotation must not keep such a result
#include "icp_solve_row.hpp"

using namespace cd;

struct RowHost {
    template <class T>
    struct V {
        T v[16];
        T& operator()(int l) { return v[l]; }
        const T& operator()(int l) const { return v[l]; }
    };
    template <class F> void each(F&& f) { for (int l = 0; l < 16; ++l) f(l); }
    template <class T> T read(const V<T>& x, int src) const { return x.v[src]; }
};

struct Rng {
    uint64_t s;
    uint64_t next() {   // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * (1.0 / 9007199254740992.0)); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Counts { long long sets = 0, stop = 0, limit = 0, eps = 0, abs_ = 0, rel = 0, open = 0, rank2 = 0, bad = 0; };

static unsigned long long fix(double v, int shift) { return (unsigned long long)std::llrint(std::ldexp(v, shift)); }
// sums whose means are mp, mq, whose covariance is (close to) sigma and whose MSE is mse, for n correspondences
static void sums_from(int n, const double mp[3], const double mq[3], const double sg[9], double mse, unsigned long long A[16]) {
    const double k = n > 0 ? n : 1;
    for (int a = 0; a < 3; ++a) { A[a] = fix(k * mp[a], FIX_SHIFT); A[3 + a] = fix(k * mq[a], FIX_SHIFT); }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[6 + 3 * a + b] = fix(k * (sg[3 * a + b] + mq[a] * mp[b]), FIX_SHIFT);
    A[15] = fix(k * mse, FIX_SHIFT_D2);
}
static void rotation(Rng& g, double R[9]) {
    const double rx = g.uni(-3.2, 3.2), ry = g.uni(-3.2, 3.2), rz = g.uni(-3.2, 3.2);
    const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
    const double M[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx};
    std::memcpy(R, M, sizeof(M));
}
static void mul3(const double A[9], const double B[9], double C[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
static IcpState state_in(Rng& g, int iters) {
    IcpState s;
    std::memset(&s, 0, sizeof(s));
    double R[9];
    rotation(g, R);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) s.Tfinal[4 * i + j] = (float)R[3 * i + j];
        s.Tfinal[4 * i + 3] = (float)g.uni(-1.0, 1.0);
    }
    s.Tfinal[15] = 1.f;
    for (int i = 0; i < 16; ++i) s.T[i] = (float)g.uni(-1.0, 1.0);
    s.prev_mse = g.below(8) == 0 ? 1.7976931348623157e308 : g.uni(0.0, 1e-3);
    s.iters = iters;
    s.status = 7;
    return s;
}

// both implementations on one set; false (and a report) on any differing bit
template <bool BOUNDED>
static bool one(const unsigned long long A[16], int n, const IcpState& in, const IcpParams& prm, Counts& c, const char* what) {
    IcpState ref = in, got = in;
    const int dref = icp_step<BOUNDED>(ref, A, n, prm);
    RowHost row;
    RowHost::V<unsigned long long> a;
    for (int l = 0; l < 16; ++l) a(l) = A[l];
    const int dgot = icp_step_row<BOUNDED>(row, got, a, n, prm);
    c.sets += 1;
    if (BOUNDED && n < ICP_MIN_CORR) c.stop += 1;
    else if (ref.iters >= prm.max_iter) c.limit += 1;
    else if (dref && std::memcmp(&ref.prev_mse, &in.prev_mse, 8) == 0) c.eps += 1;   // (the incoming prev_mse is never the new MSE here)
    else if (dref && std::fabs(ref.prev_mse - in.prev_mse) < prm.abs_mse) c.abs_ += 1;
    else if (dref) c.rel += 1;
    else c.open += 1;
    if (dref == dgot && std::memcmp(&ref, &got, sizeof(IcpState)) == 0) return true;
    if (c.bad++ == 0) {
        std::fprintf(stderr, "DIFFERENT (%s, bounded %d, n %d): done %d / %d\n", what, (int)BOUNDED, n, dref, dgot);
        for (int i = 0; i < 16; ++i) std::fprintf(stderr, "  A[%2d] %016llx  T %a / %a  Tfinal %a / %a\n", i, A[i], ref.T[i], got.T[i], ref.Tfinal[i], got.Tfinal[i]);
        std::fprintf(stderr, "  prev_mse %a / %a iters %d / %d converged %d / %d\n", ref.prev_mse, got.prev_mse, ref.iters, got.iters, ref.converged, got.converged);
    }
    return false;
}
static bool both(const unsigned long long A[16], int n, const IcpState& in, const IcpParams& prm, Counts& c, const char* what) {
    const bool x = one<false>(A, n, in, prm, c, what), y = one<true>(A, n, in, prm, c, what);
    return x && y;
}

static IcpParams params(int kind) {
    IcpParams p;
    std::memset(&p, 0, sizeof(p));
    p.max_iter = 50;
    p.trans_eps = 1e-8; p.rot_thr = 1.0 - 1e-8; p.rel_mse = 1e-6; p.abs_mse = 1e-12;   // the defaults of the library
    if (kind == 1) { p.trans_eps = 1e-3; p.rot_thr = 1.0 - 1e-3; }       // rotation / translation epsilon within reach
    if (kind == 2) { p.abs_mse = 1e-5; }                                  // absolute MSE within reach
    if (kind == 3) { p.rel_mse = 0.5; }                                   // relative MSE within reach
    if (kind == 4) { p.max_iter = 3; }
    return p;
}

static void random_sets(uint64_t seed, long long count, Counts& c) {
    Rng g{seed};
    for (long long it = 0; it < count; ++it) {
        const int kind = g.below(10);
        int n = 3 + g.below(2000);
        double mp[3], mq[3], sg[9];
        for (int a = 0; a < 3; ++a) { mp[a] = g.uni(-1.0, 1.0); mq[a] = g.uni(-1.0, 1.0); }
        for (double& v : sg) v = g.uni(-1.0, 1.0);
        double mse = g.uni(0.0, 1e-3);
        unsigned long long A[16];
        if (kind == 1) { const double s = std::pow(10.0, g.uni(-9.0, 3.0)); for (double& v : sg) v *= s; }
        if (kind == 2) { sg[3] = sg[1]; sg[6] = sg[2]; sg[7] = sg[5]; }                         // symmetric
        if (kind == 3) for (double& v : sg) if (g.below(2)) v = 0.0;                           // sparse
        if (kind == 4 || kind == 5 || kind == 6) {   // U diag V^T: equal singular values / rank 2 (either handedness) / near identity
            double U[9], V[9], D[9] = {0}, UD[9];
            rotation(g, U); rotation(g, V);
            if (kind == 4) D[0] = D[4] = D[8] = g.uni(0.01, 1.0);
            if (kind == 5) { D[0] = g.uni(0.1, 1.0); D[4] = g.uni(0.01, 0.1) * (g.below(2) ? 1.0 : -1.0); D[8] = 0.0; for (int a = 0; a < 3; ++a) mp[a] = mq[a] = 0.0; n = 1; }
            if (kind == 6) { D[0] = g.uni(0.01, 1.0); D[4] = g.uni(0.01, 1.0); D[8] = g.uni(-1.0, 1.0); std::memcpy(V, U, sizeof(U)); for (int a = 0; a < 3; ++a) mq[a] = mp[a] + g.uni(-1e-5, 1e-5); }
            mul3(U, D, UD);
            double Vt[9];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Vt[3 * i + j] = V[3 * j + i];
            mul3(UD, Vt, sg);
        }
        if (kind == 7) {   // the moments of real point pairs: q = R p + t + noise, summed the way the kernels do (rule C4)
            n = 3 + g.below(40);
            double R[9], tr[3] = {g.uni(-0.05, 0.05), g.uni(-0.05, 0.05), g.uni(-0.05, 0.05)};
            rotation(g, R);
            if (g.below(2)) { const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; std::memcpy(R, I, sizeof(I)); }
            for (auto& v : A) v = 0ull;
            for (int i = 0; i < n; ++i) {
                const float p[3] = {(float)g.uni(-0.2, 0.2), (float)g.uni(-0.1, 0.1), (float)g.uni(0.3, 0.9)};
                float q[3];
                for (int a = 0; a < 3; ++a) q[a] = (float)(R[3 * a] * p[0] + R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2] + tr[a] + g.uni(-1e-4, 1e-4));
                const float d2 = ((q[0] - p[0]) * (q[0] - p[0]) + (q[1] - p[1]) * (q[1] - p[1])) + (q[2] - p[2]) * (q[2] - p[2]);
                for (int a = 0; a < 3; ++a) {
                    A[a] += fix(p[a], FIX_SHIFT); A[3 + a] += fix(q[a], FIX_SHIFT);
                    for (int b = 0; b < 3; ++b) A[6 + 3 * a + b] += fix(q[a] * p[b], FIX_SHIFT);
                }
                A[15] += fix(d2, FIX_SHIFT_D2);
            }
        } else {
            sums_from(n, mp, mq, sg, mse, A);
        }
        const IcpParams prm = params(g.below(5));
        IcpState in = state_in(g, g.below(6));
        if (g.below(4) == 0) in.prev_mse = mse * (1.0 + g.uni(-1e-6, 1e-6));
        const int nb = g.below(50) == 0 ? g.below(4) : n;   // now and then too few correspondences for BOUNDED
        if (nb != n && kind != 7) sums_from(nb, mp, mq, sg, mse, A);
        if (kind == 7 && nb != n) continue;
        if (kind == 5) c.rank2 += 1;
        both(A, nb, in, prm, c, "random");
    }
}

static void structured(Counts& c) {
    Rng g{77};
    const double Z[3] = {0, 0, 0};
    const double mats[][9] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0},                       // zero covariance: scale == 0
        {0.5, 0, 0, 0, 0, 0, 0, 0, 0},                     // rank 1
        {0, 0, 0.25, 0, 0, 0, 0, 0, 0},                    // rank 1, off the diagonal
        {0.5, 0, 0, 0, 0.25, 0, 0, 0, 0},                  // rank 2, det U det V > 0
        {0.5, 0, 0, 0, -0.25, 0, 0, 0, 0},                 // rank 2, det U det V < 0
        {0, 0.5, 0, 0.25, 0, 0, 0, 0, 0},                  // rank 2, a permutation
        {0.5, 0, 0, 0, 0.25, 0, 0, 0, -0.125},             // det(sigma) < 0
        {-0.5, 0, 0, 0, -0.25, 0, 0, 0, -0.125},           // det(sigma) < 0, all negative
        {0.5, 0.25, 0, 0.125, -0.5, 0, 0, 0, 0.25},        // m00 + m11 == 0 in pair (1, 0)
        {0.5, 0.25, 0, -0.25, -0.5, 0, 0, 0, 0.25},        // ... with d > 0
        {0.5, 0.25, 0, 0.25, -0.5, 0, 0, 0, 0.25},         // ... with d == 0
        {0, 0.125, 0, 0, 0.5, 0, 0, 0, 0.25},              // y == 0 in make_jacobi: the block [[a, 0], [b, 0]] of pair (1, 0)
        {0.25, 0, 0, 0.125, 0, 0, 0, 0, 0.5},              // an exactly zero off-diagonal next to a non-zero one
        {0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5},                 // diagonal, equal
        {0.125, 0, 0, 0, 0.25, 0, 0, 0, 0.5},              // diagonal, ascending: the sort swaps twice
        {0.25, 0, 0, 0, 0.5, 0, 0, 0, 0.125},              // diagonal: first swap only
        {1, 1, 1, 1, 1, 1, 1, 1, 1},                       // rank 1, dense
        {1, 2, 3, 4, 5, 6, 7, 8, 9},                       // rank 2, dense
        {2147483647.0, 0, 0, 0, 1.0 / 4294967296.0, 0, 0, 0, 1},   // the largest and the smallest entry a sum can hold
        {1.0 / 4294967296.0, 1.0 / 4294967296.0, 0, 0, 1.0 / 4294967296.0, 0, 0, 0, 0},   // one unit of the sums
    };
    for (const auto& sg : mats)
        for (int kind = 0; kind < 5; ++kind)
            for (int n : {1, 2, 3, 4, 1000}) {
                unsigned long long A[16];
                sums_from(n, Z, Z, sg, 1e-4, A);
                for (int iters : {0, 2, 49}) both(A, n, state_in(g, iters), params(kind), c, "structured");
            }
    // sums at the ends of their range, n = 0 (inf and NaN means), a huge n
    const unsigned long long ends[] = {0ull, 1ull, ~0ull, 1ull << 62, (unsigned long long)(-(1ll << 62)), 0x7fffffffffffffffull, 0x8000000000000000ull};
    for (int rep = 0; rep < 4000; ++rep) {
        unsigned long long A[16];
        for (auto& v : A) v = rep < 200 ? ends[g.below(7)] : (g.below(3) ? g.next() : ends[g.below(7)]);
        const int ns[] = {0, 1, 2, 3, 7, 2147483647, -1};
        both(A, ns[g.below(7)], state_in(g, g.below(4)), params(g.below(5)), c, "extreme");
    }
    // each convergence branch by construction: identity motion (epsilon), a repeated MSE (absolute), a close one (relative)
    for (int rep = 0; rep < 200; ++rep) {
        double U[9], D[9] = {0}, UD[9], Ut[9], sg[9], mp[3] = {g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
        rotation(g, U);
        D[0] = g.uni(0.1, 1.0); D[4] = g.uni(0.1, 1.0); D[8] = g.uni(0.1, 1.0);
        mul3(U, D, UD);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Ut[3 * i + j] = U[3 * j + i];
        mul3(UD, Ut, sg);   // symmetric positive definite: R = identity
        unsigned long long A[16];
        sums_from(500, mp, mp, sg, 1e-4, A);
        for (int kind = 0; kind < 5; ++kind) {
            IcpState in = state_in(g, 1);
            both(A, 500, in, params(kind), c, "identity");
            in.prev_mse = unfix(A[15], FIX_SHIFT_D2) / 500.0;
            both(A, 500, in, params(kind), c, "same mse");
            in.prev_mse *= 1.0 + 1e-9;
            both(A, 500, in, params(kind), c, "close mse");
        }
        double mq[3] = {mp[0] + 0.01, mp[1], mp[2]};
        sums_from(500, mp, mq, sg, 1e-4, A);
        IcpState in = state_in(g, 1);
        in.prev_mse = unfix(A[15], FIX_SHIFT_D2) / 500.0;
        both(A, 500, in, params(0), c, "same mse, moving");
        in.prev_mse *= 1.0 + 1e-9;
        both(A, 500, in, params(0), c, "close mse, moving");
    }
}

int main(int argc, char** argv) {
    const long long total = argc > 1 ? std::atoll(argv[1]) : 10000000ll;
    const int nthreads = 8;
    std::vector<Counts> cs(nthreads + 1);
    structured(cs[nthreads]);
    std::vector<std::thread> th;
    for (int i = 0; i < nthreads; ++i)
        th.emplace_back([&, i] { random_sets(20190409ull + 1000003ull * (uint64_t)i, total / nthreads + (i < total % nthreads ? 1 : 0), cs[i]); });
    for (auto& t : th) t.join();
    Counts c;
    for (const Counts& x : cs) {
        c.sets += x.sets; c.stop += x.stop; c.limit += x.limit; c.eps += x.eps; c.abs_ += x.abs_; c.rel += x.rel; c.open += x.open; c.rank2 += x.rank2; c.bad += x.bad;
    }
    if (c.bad) { std::printf("FAILED %lld of %lld\n", c.bad, c.sets); return 1; }
    std::printf("ok %lld %lld %lld %lld %lld %lld %lld %lld\n", c.sets, c.stop, c.limit, c.eps, c.abs_, c.rel, c.open, c.rank2);
    return 0;
}
