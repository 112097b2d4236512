// k_depth.hip - depth image (16UC1, optionally + registered rgb8) -> organized cloud of 16-byte x y z rgb records.
//
// Canonical rule C7: z = (float)d * depth_scale, x = (((float)u - cx) / fx) * z, y = (((float)v - cy) / fy) * z,
// rgb word = (r << 16) | (g << 8) | b (0 without colour); d == 0: x = y = z = quiet NaN 0x7FC00000, rgb word as for a valid
// pixel.  Pixel (u, v) of frame f is record f * W * H + v * W + u: depth, colour and records of a batch are all tightly packed,
// so the batch is ONE linear stream of pixels and the rows' alignment does not matter (odd widths need nothing special).
//
// A workgroup takes tiles of DEP_TILE pixels: the depth (4 KiB) and colour (6 KiB) of a tile come in with one 16-byte load
// per lane (colour: 1.5 per lane), are parked in LDS, and every lane then writes pixels t, t + 256, ... of the tile, so that a
// wave's dwordx4 store covers 1 KiB of contiguous records.  A tile that is not whole (the end of the batch) or whose source
// is not 16-byte aligned (a caller's device pointer) is read element by element instead - same results.
#include <algorithm>

#include "kernels.hpp"
#include "label_math.hpp"

namespace cd {

constexpr int DEP_PER_LANE = 8;
constexpr int DEP_TILE = BLOCK * DEP_PER_LANE;   // 2048 pixels

__global__ void __launch_bounds__(BLOCK) k_deproject(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ color,
                                                     DeprojectParams dp, float4* __restrict__ out) {
    CD_FRONT_PRIO();
    __shared__ uint4 s_depth[DEP_TILE * 2 / 16];       // 256 x 16 B
    __shared__ uint4 s_color[DEP_TILE * 3 / 16];       // 384 x 16 B
    const int t = threadIdx.x;
    const uint32_t P = (uint32_t)dp.width * (uint32_t)dp.height;
    const bool vec_d = (reinterpret_cast<uintptr_t>(depth) & 15u) == 0;
    const bool vec_c = !color || (reinterpret_cast<uintptr_t>(color) & 15u) == 0;
    const uint16_t* sd = reinterpret_cast<const uint16_t*>(s_depth);
    const uint8_t* sc = reinterpret_cast<const uint8_t*>(s_color);
    for (size_t tile = blockIdx.x; tile * DEP_TILE < dp.total; tile += gridDim.x) {
        const size_t g0 = tile * DEP_TILE;
        const int n = dp.total - g0 < (size_t)DEP_TILE ? (int)(dp.total - g0) : DEP_TILE;
        // ---- stage the tile's depth and colour in LDS
        if (n == DEP_TILE && vec_d) {
            s_depth[t] = reinterpret_cast<const uint4*>(depth + g0)[t];
        } else {
            uint16_t* w = reinterpret_cast<uint16_t*>(s_depth);
            for (int j = t; j < n; j += BLOCK) w[j] = depth[g0 + j];
        }
        if (color) {
            const uint8_t* cg = color + g0 * 3;
            if (n == DEP_TILE && vec_c) {
                for (int j = t; j < DEP_TILE * 3 / 16; j += BLOCK) s_color[j] = reinterpret_cast<const uint4*>(cg)[j];
            } else {
                uint8_t* w = reinterpret_cast<uint8_t*>(s_color);
                for (int j = t; j < 3 * n; j += BLOCK) w[j] = cg[j];
            }
        }
        __syncthreads();
        // ---- position of this lane's first pixel, then steps of BLOCK pixels (= stepv rows + stepu columns, modulo the frame)
        const uint32_t p0 = (uint32_t)(g0 % P);
        uint32_t p = (p0 + (uint32_t)t) % P;
        uint32_t v = p / (uint32_t)dp.width, u = p - v * (uint32_t)dp.width;
#pragma unroll
        for (int k = 0; k < DEP_PER_LANE; ++k) {
            const int j = k * BLOCK + t;
            if (j < n) {
                const uint32_t d = sd[j];
                uint32_t rgb = 0u;
                if (color) rgb = ((uint32_t)sc[3 * j] << 16) | ((uint32_t)sc[3 * j + 1] << 8) | (uint32_t)sc[3 * j + 2];
                float4 r;
                deproject_c7(u, v, d, dp.fx, dp.fy, dp.cx, dp.cy, dp.depth_scale, &r.x, &r.y, &r.z);   // (label_math.hpp: rule C15 deprojects the same way)
                r.w = __uint_as_float(rgb);
                out[g0 + j] = r;
            }
            u += dp.stepu;
            if (u >= (uint32_t)dp.width) { u -= (uint32_t)dp.width; ++v; }
            v += dp.stepv;
            if (v >= (uint32_t)dp.height) v -= (uint32_t)dp.height;
        }
        __syncthreads();   // (the next tile overwrites the LDS)
    }
}

void launch_deproject(hipStream_t s, const uint16_t* depth, const uint8_t* color, int width, int height, int n_frames, float fx,
                      float fy, float cx, float cy, float depth_scale, float4* out) {
    DeprojectParams dp;
    dp.width = width;
    dp.height = height;
    dp.fx = fx; dp.fy = fy; dp.cx = cx; dp.cy = cy;
    dp.depth_scale = depth_scale;
    dp.total = (size_t)width * height * n_frames;
    // BLOCK pixels further on: BLOCK / W rows and BLOCK % W columns, the rows modulo H (a frame smaller than BLOCK pixels wraps)
    dp.stepu = (uint32_t)(BLOCK % width);
    dp.stepv = (uint32_t)((BLOCK / width) % height);
    if (dp.total == 0) return;
    const size_t tiles = (dp.total + DEP_TILE - 1) / DEP_TILE;
    const unsigned grid = (unsigned)std::min<size_t>(tiles, 2048);   // grid-stride beyond 8 workgroups per CU
    hipLaunchKernelGGL(k_deproject, dim3(grid), dim3(BLOCK), 0, s, depth, color, dp, out);
}

}  // namespace cd
