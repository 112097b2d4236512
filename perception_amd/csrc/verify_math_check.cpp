// verify_math_check.cpp - host-only check of verify_math.hpp (tests/test_verify_cpu.py builds and runs it; see the Makefile for a
// sanitizer build).  For a few thousand deterministic boxes - rotations in view, boxes that graze the camera plane, fill the image
// or lie off-screen, rotations that are scaled, sheared or slightly off orthonormal, non-finite poses - it counts rule C14 the
// way the kernel of k_verify.hip does (step 1, the rectangle of verify_rect, the pixels inside it) and over every pixel of the
// image, and requires the same counts: the rectangle may leave out misses only.
//
//   verify_math_check [boxes]      prints "ok <boxes> <verified> <smaller rectangles> <hits>", exit status 1 on a difference
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "verify_math.hpp"

using namespace cd;

static uint64_t g_state = 20190409ull;
static uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * (1.0 / 9007199254740992.0)); }

static void rotation(double rx, double ry, double rz, double R[9]) {
    const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
    const double M[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx};
    std::memcpy(R, M, sizeof(M));
}

static bool same(const VerifyCounts& a, const VerifyCounts& b) {
    return a.n_hit == b.n_hit && a.n_agree == b.n_agree && a.n_through == b.n_through && a.n_occluded == b.n_occluded &&
           a.n_invalid == b.n_invalid && a.agree_abs_um == b.agree_abs_um;
}

int main(int argc, char** argv) {
    const int boxes = argc > 1 ? std::atoi(argv[1]) : 4000;
    const VerifyCam cams[2] = {{70.0, 70.0, 48.0, 30.1, 0.001, 97, 61}, {96.02, 96.02, 80.6, 60.2, 0.001, 160, 120}};
    long long n_verified = 0, n_smaller = 0, n_hits = 0;
    for (int i = 0; i < boxes; ++i) {
        const VerifyCam& cam = cams[i & 1];
        const int kind = (i >> 1) % 10;
        double R[9], pose[16] = {0};
        rotation(uni(-3.2, 3.2), uni(-3.2, 3.2), uni(-3.2, 3.2), R);
        double t[3] = {uni(-0.5, 0.5), uni(-0.4, 0.4), uni(0.3, 1.5)};
        double dims[3] = {uni(0.0, 0.5), uni(0.0, 0.3), uni(0.0, 0.2)};
        if (kind == 1) t[2] = uni(0.0, 0.3);                                          // grazes the camera plane
        if (kind == 2) { dims[0] = uni(1.0, 6.0); dims[1] = uni(1.0, 6.0); }          // fills the image
        if (kind == 3) { t[0] = uni(-40.0, 40.0); t[1] = uni(-40.0, 40.0); }          // off-screen
        if (kind == 4) { const double s = (i & 2) ? uni(0.05, 1.0) : uni(1.0, 30.0); for (double& v : R) v *= s; }   // scaled
        if (kind == 5) { R[1] += uni(-0.5, 0.5); R[5] += uni(-0.5, 0.5); }            // sheared
        if (kind == 6) for (double& v : R) v += uni(-3e-4, 3e-4);                     // off orthonormal, inside the 1e-3 of verify_rect
        if (kind == 7) for (double& v : R) v += uni(-2e-3, 2e-3);                     // ... and around it
        if (kind == 8) { rotation(0.0, 0.0, 0.0, R); t[0] = 0.0; t[2] = uni(0.5, 1.0); }   // axis-aligned on the column u = cx
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) pose[4 * r + c] = R[3 * r + c];
            pose[4 * r + 3] = t[r];
        }
        pose[15] = 1.0;
        if (kind == 9) pose[(next_u64() % 3) * 4 + next_u64() % 4] = (i & 2) ? NAN : INFINITY;
        const double tau = 0.01;
        VerifySetup s;
        verify_setup(pose, dims, &s);
        if (!s.verified) continue;
        ++n_verified;
        // the depth image: around the rendered depth where the box is hit, 0 / 1 / 65535 elsewhere
        std::vector<uint16_t> depth((size_t)cam.width * cam.height);
        for (int v = 0; v < cam.height; ++v)
            for (int u = 0; u < cam.width; ++u) {
                double z;
                const uint64_t r = next_u64();
                uint16_t d = (uint16_t)((r & 3) == 0 ? 0 : (r & 3) == 1 ? 1 : 65535);
                if (verify_hit(s, cam, u, v, &z) && (r & 4)) {
                    const double q = floor(z / cam.depth_scale + 0.5) + (double)((int)((r >> 3) % 7) - 3) * 4.0;
                    if (q >= 0.0 && q <= 65535.0) d = (uint16_t)q;
                }
                depth[(size_t)v * cam.width + u] = d;
            }
        VerifyCounts whole = {0, 0, 0, 0, 0, 0ull}, part = {0, 0, 0, 0, 0, 0ull};
        double z;
        for (int v = 0; v < cam.height; ++v)
            for (int u = 0; u < cam.width; ++u) verify_pixel(s, cam, tau, u, v, depth[(size_t)v * cam.width + u], &z, &whole);
        int32_t x0, y0, x1, y1;
        verify_rect(s, pose, cam, &x0, &y0, &x1, &y1);
        if (x0 <= x1 && y0 <= y1 && (x0 < 0 || y0 < 0 || x1 >= cam.width || y1 >= cam.height)) {
            std::fprintf(stderr, "box %d: rectangle %d %d %d %d leaves the image\n", i, x0, y0, x1, y1);
            return 1;
        }
        for (int v = y0; v <= y1; ++v)
            for (int u = x0; u <= x1; ++u) verify_pixel(s, cam, tau, u, v, depth[(size_t)v * cam.width + u], &z, &part);
        if (!same(whole, part)) {
            std::fprintf(stderr, "box %d (kind %d): the rectangle %d %d %d %d holds %d of %d hits\n", i, kind, x0, y0, x1, y1, part.n_hit, whole.n_hit);
            return 1;
        }
        n_hits += whole.n_hit;
        n_smaller += (x1 - x0 + 1) < cam.width || (y1 - y0 + 1) < cam.height || x0 > x1 || y0 > y1;
    }
    std::printf("ok %d %lld %lld %lld\n", boxes, n_verified, n_smaller, n_hits);
    return 0;
}
