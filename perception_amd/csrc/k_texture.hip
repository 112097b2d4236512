// k_texture.hip - unregistered depth image (16UC1) + colour image (rgb8, its own size and intrinsics) + depth->colour extrinsics
// -> organized cloud of 16-byte x y z rgb records, in the DEPTH camera's frame, each point coloured by the colour pixel it
// projects to.  Canonical rule C12 (texture_math.hpp holds the arithmetic, shared with cd_texture_project).
//
// Pixel (u, v) of depth frame f is record f * W * H + v * W + u: depth and records of a batch are one linear stream of pixels,
// as in k_depth.hip, and the tile shape is the same: a workgroup takes tiles of TEX_TILE pixels, the depth of a tile (4 KiB)
// comes in with one 16-byte load per lane and is parked in LDS, and every lane then writes pixels t, t + 256, ... of the tile,
// so that a wave's dwordx4 store covers 1 KiB of contiguous records.  A tile that is not whole or whose source is not 16-byte
// aligned is read element by element instead - same results.
//
// The colour is a GATHER: 3 bytes of frame f's colour image per textured point.  Neighbouring lanes hold neighbouring depth
// pixels, which project to neighbouring colour pixels (the same one, or the next, for the D435 pair), so a wave's three byte
// loads fall into a few cache lines it has already touched; the colour is not staged in LDS.  The frame of a pixel comes from
// its position in the stream.
#include <algorithm>

#include "kernels.hpp"
#include "texture_math.hpp"

namespace cd {

constexpr int TEX_PER_LANE = 8;
constexpr int TEX_TILE = BLOCK * TEX_PER_LANE;   // 2048 pixels

struct TextureLaunch {
    TextureParams tp;
    uint32_t width, height;   // depth image
    uint32_t stepu, stepv;    // BLOCK pixels further on inside a frame: columns, rows
    size_t total;             // depth pixels of the batch
    size_t color_frame;       // bytes of one colour image
};

__global__ void __launch_bounds__(BLOCK) k_texture_map(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ color,
                                                       TextureLaunch tl, float4* __restrict__ out) {
    CD_FRONT_PRIO();
    __shared__ uint4 s_depth[TEX_TILE * 2 / 16];       // 256 x 16 B
    const int t = threadIdx.x;
    const uint32_t W = tl.width, P = tl.width * tl.height;
    const bool vec_d = (reinterpret_cast<uintptr_t>(depth) & 15u) == 0;
    const uint16_t* sd = reinterpret_cast<const uint16_t*>(s_depth);
    for (size_t tile = blockIdx.x; tile * TEX_TILE < tl.total; tile += gridDim.x) {
        const size_t g0 = tile * TEX_TILE;
        const int n = tl.total - g0 < (size_t)TEX_TILE ? (int)(tl.total - g0) : TEX_TILE;
        // ---- stage the tile's depth in LDS
        if (n == TEX_TILE && vec_d) {
            s_depth[t] = reinterpret_cast<const uint4*>(depth + g0)[t];
        } else {
            uint16_t* w = reinterpret_cast<uint16_t*>(s_depth);
            for (int j = t; j < n; j += BLOCK) w[j] = depth[g0 + j];
        }
        __syncthreads();
        // ---- frame and position of this lane's first pixel, then steps of BLOCK pixels
        const size_t g = g0 + (size_t)t;
        size_t f = tl.total <= 0xffffffffull ? (size_t)((uint32_t)g / P) : g / P;   // (a 64-bit division only for batches that need one)
        uint32_t p = (uint32_t)(g - f * P);
        uint32_t v = p / W, u = p - v * W;
#pragma unroll
        for (int k = 0; k < TEX_PER_LANE; ++k) {
            const int j = k * BLOCK + t;
            if (j < n) {
                float xyz[3];
                int32_t pix[2];
                uint32_t rgb = 0u;
                if (texture_point(tl.tp, u, v, sd[j], xyz, pix)) {   // (0 <= pix < cw, ch: inside frame f's colour image)
                    const uint8_t* c = color + f * tl.color_frame + ((size_t)pix[1] * (size_t)tl.tp.cw + (size_t)pix[0]) * 3;
                    rgb = ((uint32_t)c[0] << 16) | ((uint32_t)c[1] << 8) | (uint32_t)c[2];
                }
                float4 r;
                r.x = xyz[0]; r.y = xyz[1]; r.z = xyz[2];
                r.w = __uint_as_float(rgb);
                out[g0 + j] = r;
            }
            p += BLOCK;
            if (p >= P) {   // into a later frame (several frames on when a frame is smaller than BLOCK pixels)
                do { p -= P; ++f; } while (p >= P);
                v = p / W;
                u = p - v * W;
            } else {
                u += tl.stepu;
                v += tl.stepv;
                if (u >= W) { u -= W; ++v; }
            }
        }
        __syncthreads();   // (the next tile overwrites the LDS)
    }
}

void launch_texture_map(hipStream_t s, const uint16_t* depth, const uint8_t* color, int width, int height, int n_frames,
                        const TextureParams& tp, float4* out) {
    TextureLaunch tl;
    tl.tp = tp;
    tl.width = (uint32_t)width;
    tl.height = (uint32_t)height;
    tl.stepu = (uint32_t)(BLOCK % width);
    tl.stepv = (uint32_t)(BLOCK / width);
    tl.total = (size_t)width * height * n_frames;
    tl.color_frame = (size_t)tp.cw * tp.ch * 3;
    if (tl.total == 0) return;
    const size_t tiles = (tl.total + TEX_TILE - 1) / TEX_TILE;
    const unsigned grid = (unsigned)std::min<size_t>(tiles, 2048);   // grid-stride beyond 8 workgroups per CU
    hipLaunchKernelGGL(k_texture_map, dim3(grid), dim3(BLOCK), 0, s, depth, color, tl, out);
}

}  // namespace cd
