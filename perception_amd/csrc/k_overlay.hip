// k_overlay.hip - canonical rule C11: the projected ICP boxes of cuboid_detection/scripts/draw_bbox.py:44-83,
// drawn into the rgb8 images of a batch where they lie in device memory.
//
// k_overlay_project: one lane per corner, eight lanes per box.  Steps 1, 3 and 4 of the rule (overlay_math.hpp: float32 corner,
// double projection with explicit round-to-nearest operations, truncation, the skip tests); a box is drawn iff all its eight
// lanes say so (one ballot per wave), and a skipped or absent box leaves an all-zero record.
//
// k_overlay_raster: one WAVE per (frame, box, edge), four edges per workgroup.  An edge covers the bounding rectangle of its two
// end points grown by ceil(t / 2) and clipped to the image; the wave walks the rectangle's rows, and within a row only the
// columns that can lie within ceil(t / 2) of the part of the segment within ceil(t / 2) rows of it (a superset of the painted
// pixels, so the exact test below decides alone).  Lane i takes pixel x0 + i of the row: the three byte stores of a wave cover
// 192 contiguous bytes.  The test of step 6 runs in int64 and is the whole of the arithmetic; painted pixels get plain byte
// stores of the call's one colour, so edges (and boxes) that overlap write identical bytes and need no ordering.  Every loop
// is bounded by the clipped rectangle: at most 8192 rows of at most 8192 / 64 steps.
//
// Launch shape: the work per edge is a few hundred pixel tests, so the kernel is latency- and not throughput-bound; 256-thread
// workgroups of four independent waves (no LDS, no barrier; compiler report: 81 VGPRs, no scratch, 5 waves per SIMD) keep up to 20
// edges in flight per CU.
#include "kernels.hpp"
#include "overlay_math.hpp"

namespace cd {

__global__ void __launch_bounds__(BLOCK) k_overlay_project(const double* __restrict__ poses, const int32_t* __restrict__ n_boxes, int B,
                                                           int total_boxes, OverlayParams op, OverlayBox* __restrict__ out) {
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    const int box = gid >> 3, k = gid & 7;
    bool ok = false;
    int32_t u = 0, v = 0;
    if (box < total_boxes) {
        const int f = box / B, b = box - f * B;
        if (b < n_boxes[f]) {
            float c[3];
            overlay_corner(poses + (size_t)box * 16, op.dims, k, c);
            ok = overlay_pixel(op.M, c, &u, &v);
        }
    }
    // the eight lanes of a box are consecutive lanes of one wave (BLOCK and the wave size are multiples of 8); every lane of
    // the wave reaches the ballot
    const unsigned long long m = __ballot(ok);
    const int lane = threadIdx.x & 63;
    const bool drawn = ((m >> (lane & ~7)) & 0xffull) == 0xffull;
    if (box < total_boxes) {
        OverlayBox* o = out + box;
        o->corners[2 * k] = drawn ? u : 0;
        o->corners[2 * k + 1] = drawn ? v : 0;
        if (k == 0) o->drawn = drawn ? 1 : 0;
        if (k >= 1 && k <= 3) o->reserved[k - 1] = 0;
    }
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}

__global__ void __launch_bounds__(BLOCK) k_overlay_raster(uint8_t* __restrict__ img, int W, int H, int B, int total_edges, int thickness,
                                                          uint32_t rgb, const OverlayBox* __restrict__ boxes) {
    const int item = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);   // (frame, box, edge), wave-uniform
    if (item >= total_edges) return;
    const int lane = threadIdx.x & 63;
    const int box = item / 12, e = item - box * 12;
    const OverlayBox* ob = boxes + box;
    if (!ob->drawn) return;
    // the 12 corner pairs of draw_bbox.py:66-77, in that order, as two nibble strings
    const unsigned long long EA = 0x654432211000ull, EB = 0x776576353421ull;
    const int ca = (int)((EA >> (4 * e)) & 15), cb = (int)((EB >> (4 * e)) & 15);
    const long long ax = ob->corners[2 * ca], ay = ob->corners[2 * ca + 1];
    const long long bx = ob->corners[2 * cb], by = ob->corners[2 * cb + 1];
    const long long r = (thickness + 1) / 2;
    const long long t2 = (long long)thickness * thickness;
    const long long dx = bx - ax, dy = by - ay, L = dx * dx + dy * dy;
    // clipped rectangle (empty: nothing to do)
    const long long xlo = max(min(ax, bx) - r, 0ll), xhi = min(max(ax, bx) + r, (long long)W - 1);
    const long long ylo = max(min(ay, by) - r, 0ll), yhi = min(max(ay, by) + r, (long long)H - 1);
    if (xlo > xhi || ylo > yhi) return;
    const int f = box / B;
    uint8_t* frame = img + (size_t)f * (size_t)W * (size_t)H * 3;
    const uint8_t c0 = (uint8_t)(rgb & 255u), c1 = (uint8_t)((rgb >> 8) & 255u), c2 = (uint8_t)((rgb >> 16) & 255u);
    // the segment's lower and upper end in y, for the per-row column bounds
    const long long sy0 = min(ay, by), sy1 = max(ay, by);
    const long long ady = dy < 0 ? -dy : dy, sdx = dy < 0 ? -dx : dx;         // direction with a non-negative y step
    const long long ox = dy < 0 ? bx : ax;                                    // x of the end with the smaller y (= sy0)
    for (long long y = ylo; y <= yhi; ++y) {
        long long x0 = xlo, x1 = xhi;
        if (ady != 0) {
            // the part of the segment with |y' - y| <= r: x runs between its values at ya and yb
            const long long ya = max(y - r, sy0), yb = min(y + r, sy1);       // ya <= yb: y is within r of [sy0, sy1]
            const long long na = (ya - sy0) * sdx, nb = (yb - sy0) * sdx;     // x = ox + n / ady
            const long long lo = ox + floor_div(min(na, nb), ady), hi = ox + ceil_div(max(na, nb), ady);
            x0 = max(x0, lo - r);
            x1 = min(x1, hi + r);
        }
        uint8_t* row = frame + (size_t)y * (size_t)W * 3;
        const long long ey = y - ay, fy = y - by;
        for (long long xs = x0; xs <= x1; xs += 64) {
            const long long x = xs + lane;
            if (x > x1) continue;
            const long long ex = x - ax;
            const long long s = ex * dx + ey * dy;
            bool paint;
            if (L == 0 || s <= 0) {
                paint = 4 * (ex * ex + ey * ey) <= t2;
            } else if (s >= L) {
                const long long fx = x - bx;
                paint = 4 * (fx * fx + fy * fy) <= t2;
            } else {
                const long long cr = ex * dy - ey * dx;
                paint = 4 * (cr * cr) <= t2 * L;
            }
            if (paint) {
                uint8_t* p = row + (size_t)x * 3;
                p[0] = c0;
                p[1] = c1;
                p[2] = c2;
            }
        }
    }
}

void launch_overlay_project(hipStream_t s, const double* poses, const int32_t* n_boxes, int B, int F, const OverlayParams& op, OverlayBox* out) {
    const long long total = (long long)F * B;
    if (total <= 0) return;
    const unsigned grid = (unsigned)((total * 8 + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_overlay_project, dim3(grid), dim3(BLOCK), 0, s, poses, n_boxes, B, (int)total, op, out);
}

void launch_overlay_raster(hipStream_t s, uint8_t* img, int W, int H, int B, int F, int thickness, const uint8_t rgb[3], const OverlayBox* boxes) {
    const long long edges = (long long)F * B * 12;
    if (edges <= 0) return;
    const unsigned grid = (unsigned)((edges + BLOCK / 64 - 1) / (BLOCK / 64));
    const uint32_t packed = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    hipLaunchKernelGGL(k_overlay_raster, dim3(grid), dim3(BLOCK), 0, s, img, W, H, B, (int)edges, thickness, packed, boxes);
}

}  // namespace cd
