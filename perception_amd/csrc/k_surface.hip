// k_surface.hip - the device side of the batched surface-normal estimation (cd_surface_batch, CD_GUESS_SURFACE).
//
// surface_normal_estimation.cpp:167-234 fits three axis-constrained planes one after the other, each to what the previous fit
// left over.  The fits themselves are S2/S3 (k_plane.hip) over the stage's own buffers; what is new here is the load of the
// clouds into those buffers and pcl::compute3DCentroid of each fit's plane points: a SEQUENTIAL float32 sum in input-index
// order (rule C6), so that a batch gives cd_surface_frame's midpoints bit for bit.  One workgroup per frame: the points of a
// chunk are tested in parallel and compacted through LDS, then one lane adds the selected ones in order.
#include <algorithm>

#include "kernels.hpp"

namespace cd {

// frame f: records of `stride` bytes at in + f * fpitch, count[f * count_pitch] of them (at most `pitch`) -> out[f * pitch + i] =
// (x, y, z, 0), as cd_surface_frame uploads a cloud
__global__ void __launch_bounds__(BLOCK) k_surface_load(const char* __restrict__ in, size_t stride, size_t fpitch,
                                                        const int* __restrict__ count, int count_pitch, int pitch,
                                                        float4* __restrict__ out) {
    CD_FRONT_PRIO();
    const int f = blockIdx.y;
    const int m = min(count[(size_t)f * count_pitch], pitch);
    const char* src = in + (size_t)f * fpitch;
    float4* dst = out + (size_t)f * pitch;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < m; i += gridDim.x * BLOCK) {
        const uint32_t* r = reinterpret_cast<const uint32_t*>(src + (size_t)i * stride);
        dst[i] = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), 0.f);
    }
}

// getNormal's plane_pc = ExtractIndices(negative = !invert) of the fit's inliers: the points whose inlier test (S3's, with
// the refined model and the have flag S3 used) equals `invert`.  out[f * out_pitch] = (sum x, sum y, sum z, count as int bits),
// the sums sequential in index order; the host divides (sne.cpp: one division per component, 0 / 0 included).
__global__ void __launch_bounds__(BLOCK) k_surface_centroid(const float4* __restrict__ pts, int pitch, const FrameState* __restrict__ fs,
                                                            const float4* __restrict__ model, const int* __restrict__ have, float thr,
                                                            int invert, float4* __restrict__ out, int out_pitch) {
    CD_FRONT_PRIO();
    __shared__ float4 s_p[BLOCK];
    __shared__ int s_wcnt[WAVES_PER_BLOCK];
    const int f = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(fs[f].n_v, pitch);
    const float4 m = model[f];
    const int hv = have[f];
    const float4* P = pts + (size_t)f * pitch;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int cnt = 0;
    for (int base = 0; base < n; base += BLOCK) {
        const int i = base + threadIdx.x;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        bool sel = false;
        if (i < n) {
            p = P[i];
            const bool inl = hv && plane_dist(m.x, m.y, m.z, m.w, p.x, p.y, p.z) < thr;
            sel = inl == (invert != 0);
        }
        const uint64_t b = __ballot(sel);
        if (lane == 0) s_wcnt[w] = __popcll(b);
        __syncthreads();
        int pos = 0;
        for (int q = 0; q < w; ++q) pos += s_wcnt[q];
        if (sel) s_p[pos + __popcll(b & lanemask_lt())] = p;   // (order kept: waves in order, lanes in order)
        int tot = 0;
        for (int q = 0; q < WAVES_PER_BLOCK; ++q) tot += s_wcnt[q];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < tot; ++k) {
                const float4 q = s_p[k];
                sx = __fadd_rn(sx, q.x);
                sy = __fadd_rn(sy, q.y);
                sz = __fadd_rn(sz, q.z);
            }
            cnt += tot;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)f * out_pitch] = make_float4(sx, sy, sz, __int_as_float(cnt));
}

void launch_surface_load(hipStream_t s, const void* in, size_t stride, size_t fpitch, const int* count, int count_pitch, int pitch,
                         int max_count, int F, float4* out) {
    const int gx = std::max(1, std::min(64, (std::min(max_count, pitch) + BLOCK - 1) / BLOCK));
    if (F > 0 && max_count > 0)
        hipLaunchKernelGGL(k_surface_load, dim3(gx, F), dim3(BLOCK), 0, s, (const char*)in, stride, fpitch, count, count_pitch, pitch, out);
}
void launch_surface_centroid(hipStream_t s, const float4* pts, int pitch, int F, const FrameState* fs, const float4* model,
                             const int* have, float thr, int invert, float4* out, int out_pitch) {
    if (F > 0) hipLaunchKernelGGL(k_surface_centroid, dim3(F), dim3(BLOCK), 0, s, pts, pitch, fs, model, have, thr, invert, out, out_pitch);
}

}  // namespace cd
