// k_verify.hip - canonical rule C14: the cuboid of every pose of a batch rendered into the 16UC1 depth image of its
// frame, and each covered pixel sorted into AGREE / THROUGH / OCCLUDED / INVALID against the depth the sensor measured there.
//
// One 256-thread workgroup per (frame, slot).  A slot at or beyond the frame's box count writes its all-zero record and leaves.
// Lane 0 computes what is uniform over the box (verify_math.hpp: the columns of R, the ray origin in the box frame, the step-1
// test, the clipped pixel rectangle of step 6) and hands it to the others through LDS.  The rectangle's pixels are then walked
// in row-major order, pixel i of the rectangle by thread i mod 256: the uint16 loads of a wave are contiguous within a row.
// Each pixel costs eight IEEE double divisions (two for the ray, two per slab) and no memory beyond its two bytes, so the kernel
// is bound by the double-precision vector rate; five int32 counters and one 64-bit sum per lane stay in registers, are folded inside each wave by shuffles (common.hpp) and across the four waves through LDS, and thread 0
// writes the record with ordinary stores.  All sums are integers: no order of summation can change a bit.  No atomics, no
// global scratch; the pixel loop is bounded by the rectangle, which the clamps of verify_rect keep inside the image.
#include "kernels.hpp"
#include "verify_math.hpp"

namespace cd {

__global__ void __launch_bounds__(BLOCK) k_verify_boxes(const uint16_t* __restrict__ depth, VerifyCam cam, double tau,
                                                        const VerifyJob* __restrict__ jobs, const int32_t* __restrict__ n_boxes, int B,
                                                        VerifyRecord* __restrict__ out) {
    __shared__ VerifySetup s_set;
    __shared__ int32_t s_rect[4];
    __shared__ unsigned long long s_part[WAVES_PER_BLOCK][6];
    const int box = blockIdx.x, f = box / B, b = box - f * B;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    VerifyRecord rec = {0, 0, 0, 0, 0, 0, 0, 0, 0ll, 0.0};
    if (b >= n_boxes[f]) {   // (uniform over the workgroup)
        if (threadIdx.x == 0) out[box] = rec;
        return;
    }
    if (threadIdx.x == 0) {
        const VerifyJob* j = jobs + box;
        verify_setup(j->pose, j->dims, &s_set);
        s_rect[0] = 0; s_rect[1] = 0; s_rect[2] = -1; s_rect[3] = -1;
        if (s_set.verified) verify_rect(s_set, j->pose, cam, &s_rect[0], &s_rect[1], &s_rect[2], &s_rect[3]);
    }
    __syncthreads();
    const VerifySetup s = s_set;
    const int x0 = s_rect[0], y0 = s_rect[1], x1 = s_rect[2], y1 = s_rect[3];
    VerifyCounts acc = {0, 0, 0, 0, 0, 0ull};
    if (x0 <= x1 && y0 <= y1) {   // 0 <= x0 <= x1 <= width - 1, 0 <= y0 <= y1 <= height - 1
        const uint16_t* __restrict__ frame = depth + (size_t)f * (size_t)cam.width * (size_t)cam.height;
        const unsigned rw = (unsigned)(x1 - x0 + 1), total = rw * (unsigned)(y1 - y0 + 1);   // <= width * height <= INT_MAX
        for (unsigned i = threadIdx.x; i < total; i += BLOCK) {
            const unsigned ry = i / rw, rx = i - ry * rw;
            const int u = x0 + (int)rx, v = y0 + (int)ry;
            const uint16_t d = frame[(size_t)v * (size_t)cam.width + (size_t)u];
            double z_r;
            verify_pixel(s, cam, tau, u, v, d, &z_r, &acc);
        }
    }
    const int n_hit = wave_sum_i32(acc.n_hit), n_agree = wave_sum_i32(acc.n_agree), n_through = wave_sum_i32(acc.n_through);
    const int n_occluded = wave_sum_i32(acc.n_occluded), n_invalid = wave_sum_i32(acc.n_invalid);
    const unsigned long long um = wave_sum_u64(acc.agree_abs_um);
    if (lane == 0) {
        s_part[w][0] = (unsigned long long)(unsigned)n_hit;
        s_part[w][1] = (unsigned long long)(unsigned)n_agree;
        s_part[w][2] = (unsigned long long)(unsigned)n_through;
        s_part[w][3] = (unsigned long long)(unsigned)n_occluded;
        s_part[w][4] = (unsigned long long)(unsigned)n_invalid;
        s_part[w][5] = um;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        for (int q = 0; q < WAVES_PER_BLOCK; ++q)
            for (int k = 0; k < 6; ++k) t[k] += s_part[q][k];
        rec.verified = s.verified;
        rec.n_hit = (int32_t)t[0];
        rec.n_agree = (int32_t)t[1];
        rec.n_through = (int32_t)t[2];
        rec.n_occluded = (int32_t)t[3];
        rec.n_invalid = (int32_t)t[4];
        rec.agree_abs_um = (long long)t[5];
        out[box] = rec;   // (score and passed are the host's: step 5)
    }
}

void launch_verify_boxes(hipStream_t s, const uint16_t* depth, const VerifyCam& cam, double tau, const VerifyJob* jobs, const int32_t* n_boxes,
                         int B, int F, VerifyRecord* out) {
    const long long total = (long long)F * B;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_verify_boxes, dim3((unsigned)total), dim3(BLOCK), 0, s, depth, cam, tau, jobs, n_boxes, B, out);
}

}  // namespace cd
