// rn_ops.hpp - ONE correctly rounded IEEE operation per call, the same on host and device (canonical rule C1): what
// the *_math.hpp headers are written in, so that a kernel and its host twin run the same sequence of roundings.  On the device
// every function is the explicit round-to-nearest intrinsic: no contraction can enter whatever the compile flags.  On the host it
// is the plain operator, which is the same operation ONLY under -ffp-contract=off -fno-fast-math - the library's FLAGS and the
// CHECK_FLAGS of the Makefile both have them.  A float square root is IEEE on the device under
// -fhip-fp32-correctly-rounded-divide-sqrt (__fsqrt_rn is the native approximation, so sqrtf it is).
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

namespace cd {

#ifdef __HIP_DEVICE_COMPILE__
__host__ __device__ inline float rn_fadd(float a, float b) { return __fadd_rn(a, b); }
__host__ __device__ inline float rn_fsub(float a, float b) { return __fsub_rn(a, b); }
__host__ __device__ inline float rn_fmul(float a, float b) { return __fmul_rn(a, b); }
__host__ __device__ inline float rn_fsqrt(float a) { return sqrtf(a); }
__host__ __device__ inline double rn_dadd(double a, double b) { return __dadd_rn(a, b); }
__host__ __device__ inline double rn_dsub(double a, double b) { return __dsub_rn(a, b); }
__host__ __device__ inline double rn_dmul(double a, double b) { return __dmul_rn(a, b); }
__host__ __device__ inline double rn_ddiv(double a, double b) { return __ddiv_rn(a, b); }
__host__ __device__ inline double rn_dsqrt(double a) { return __dsqrt_rn(a); }
__host__ __device__ inline double rn_ll2d(long long a) { return __ll2double_rn(a); }
#else
__host__ __device__ inline float rn_fadd(float a, float b) { return a + b; }
__host__ __device__ inline float rn_fsub(float a, float b) { return a - b; }
__host__ __device__ inline float rn_fmul(float a, float b) { return a * b; }
__host__ __device__ inline float rn_fsqrt(float a) { return std::sqrt(a); }
__host__ __device__ inline double rn_dadd(double a, double b) { return a + b; }
__host__ __device__ inline double rn_dsub(double a, double b) { return a - b; }
__host__ __device__ inline double rn_dmul(double a, double b) { return a * b; }
__host__ __device__ inline double rn_ddiv(double a, double b) { return a / b; }
__host__ __device__ inline double rn_dsqrt(double a) { return std::sqrt(a); }
__host__ __device__ inline double rn_ll2d(long long a) { return (double)a; }
#endif

// canonical squared distance: (dx*dx + dy*dy) + dz*dz, no contraction
__host__ __device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return rn_fadd(rn_fadd(rn_fmul(dx, dx), rn_fmul(dy, dy)), rn_fmul(dz, dz));
}
// row r of the row-major 4 x 4 matrix T on the point (x, y, z): ((T[4r] x + T[4r+1] y) + T[4r+2] z) + T[4r+3] - the single
// evaluation cd_get_cluster_points has
__host__ __device__ inline float xform_row(const float* T, int r, float x, float y, float z) {
    return rn_fadd(rn_fadd(rn_fadd(rn_fmul(T[4 * r], x), rn_fmul(T[4 * r + 1], y)), rn_fmul(T[4 * r + 2], z)), T[4 * r + 3]);
}

}  // namespace cd
