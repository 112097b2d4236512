// pose_info_math_check.cpp - host-only run of canonical rule C23 through pose_info_math.hpp (tests/test_pose_info_cpu.py builds and
// runs it and compares what it prints with perception_amd/pose_info.py).
//
//   pose_info_math_check <file>
// <file>: int32 m, int32 n, int32 accepted, int32 0, float32 T[16], double max_range, double min_support, then m * 3 float32 (the
// template, x y z) and n * 3 float32 (the cluster as extracted), little endian.  Prints two lines:
//   counts <n_source n_in n_face[0] n_face[1] n_face[2] n_constrained well_posed status>
//   values <89 words of 16 hex digits: the bits of eigenvalues[6] eigenvectors[36] weakest[6] sigma2 covariance[36] centre[3] length>
// Exit status 2 for a file it cannot read or a setting outside the rule's range.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "template_prep.hpp"
#include "pose_info_math.hpp"

using namespace cd;

// rule C8's tau (cd_icp_correspondence_threshold's arithmetic: this program links no library)
static float tau_of(double d) {
    const double dd = d * d;
    float f = (float)dd;
    if ((double)f > dd) f = std::nextafter(f, 0.f);
    return f;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: pose_info_math_check <file>\n"); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t head[4];
    float T[16];
    double lim[2];
    if (std::fread(head, sizeof(int32_t), 4, fp) != 4 || std::fread(T, sizeof(float), 16, fp) != 16 || std::fread(lim, sizeof(double), 2, fp) != 2) { std::fclose(fp); return 2; }
    const int m = head[0], n = head[1];
    if (m < 0 || m > (1 << 24) || n < 0 || n > (1 << 24) || !pose_setting_ok(lim[0], lim[1])) { std::fclose(fp); return 2; }
    std::vector<float> tpl((size_t)m * 3), src((size_t)n * 3);
    if ((m > 0 && std::fread(tpl.data(), sizeof(float), tpl.size(), fp) != tpl.size()) || (n > 0 && std::fread(src.data(), sizeof(float), src.size(), fp) != src.size())) { std::fclose(fp); return 2; }
    std::fclose(fp);

    auto L = std::make_unique<IcpLattice>();
    L->nface = 0;
    if (m > 0) lattice_detect(tpl.data(), m, L.get());
    cd_pose_info rec;
    const int pre = pose_pre_status(m, L->nface, T);
    if (pre != CD_OK) {
        pose_empty(n, pre, 0, 0, 0, 0, &rec);
    } else {
        std::vector<int> face_w((size_t)m, 0);
        pose_face_axes(*L, m, face_w.data());
        float c0[3];
        double length;
        pose_box(tpl.data(), m, c0, &length);
        long long S[POSE_NSUMS];
        int nf[3], bad;
        pose_passes_host(tpl.data(), m, face_w.data(), src.data(), n, T, tau_of(lim[0]), c0, S, nf, &bad);
        double ws[POSE_WS];
        pose_finish(n, bad, nf[0], nf[1], nf[2], S, c0[0], c0[1], c0[2], length, lim[1], head[2] ? 1 : 0, ws, &rec);
    }
    std::printf("counts %d %d %d %d %d %d %d %d\nvalues", rec.n_source, rec.n_in, rec.n_face[0], rec.n_face[1], rec.n_face[2], rec.n_constrained, rec.well_posed, rec.status);
    std::vector<double> v;
    v.insert(v.end(), rec.eigenvalues, rec.eigenvalues + 6);
    v.insert(v.end(), rec.eigenvectors, rec.eigenvectors + 36);
    v.insert(v.end(), rec.weakest, rec.weakest + 6);
    v.push_back(rec.sigma2);
    v.insert(v.end(), rec.covariance, rec.covariance + 36);
    v.insert(v.end(), rec.centre, rec.centre + 3);
    v.push_back(rec.length);
    for (double d : v) { uint64_t b; std::memcpy(&b, &d, 8); std::printf(" %016llx", (unsigned long long)b); }
    std::printf("\n");
    return 0;
}
