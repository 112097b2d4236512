// texture_math.hpp - steps 1 to 6 of canonical rule C12 for one depth pixel, shared by the host entry
// cd_texture_project and the mapping kernel of k_texture.hip so that both run the same sequence of correctly rounded float32
// operations: one IEEE operation per operator, which the library's flags guarantee on both sides (-ffp-contract=off, correctly
// rounded float32 divide on the device).
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace cd {

// both cameras of a mapped call (cd_depth_camera + cd_color_camera, as the kernel takes them by value)
struct TextureParams {
    float fx, fy, cx, cy, depth_scale;   // depth camera (rule C7)
    float cfx, cfy, ccx, ccy;            // colour camera
    float R[9], t[3];                    // p_colour = R p_depth + t, R row-major
    int32_t cw, ch;                      // colour image
    int32_t keep;                        // CD_NOTEX_KEEP: an untextured point keeps its xyz
};

__host__ __device__ inline float texture_qnan() {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(0x7FC00000u);
#else
    const uint32_t q = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &q, 4);
    return f;
#endif
}

// Pixel (u, v) with depth value d: xyz as the record holds it, pix = (iu, iv) of the colour pixel whose rgb the record takes,
// (-1, -1) and `false` when the point is not textured (its rgb word is 0).
__host__ __device__ inline bool texture_point(const TextureParams& k, uint32_t u, uint32_t v, uint32_t d, float xyz[3], int32_t pix[2]) {
    pix[0] = pix[1] = -1;
    if (d == 0u) {   // step 1
        xyz[0] = xyz[1] = xyz[2] = texture_qnan();
        return false;
    }
    // step 2: rule C7
    const float z = (float)d * k.depth_scale;
    const float x = (((float)u - k.cx) / k.fx) * z;
    const float y = (((float)v - k.cy) / k.fy) * z;
    // step 3: into the colour frame
    const float Xc = ((k.R[0] * x + k.R[1] * y) + k.R[2] * z) + k.t[0];
    const float Yc = ((k.R[3] * x + k.R[4] * y) + k.R[5] * z) + k.t[1];
    const float Zc = ((k.R[6] * x + k.R[7] * y) + k.R[8] * z) + k.t[2];
    // step 4: projection, pixel centres at integer coordinates
    const float pu = (Xc / Zc) * k.cfx + k.ccx;
    const float pv = (Yc / Zc) * k.cfy + k.ccy;
    const float fu = floorf(pu + 0.5f), fv = floorf(pv + 0.5f);
    // step 5 (written so that a NaN fails; the bounds are compared in double, where an int32 size is exact)
    const bool fin = fabsf(pu) <= 3.402823466e+38f && fabsf(pv) <= 3.402823466e+38f;
    const bool tex = Zc > 0.f && fin && (double)fu >= 0.0 && (double)fu < (double)k.cw && (double)fv >= 0.0 && (double)fv < (double)k.ch;
    if (tex) {
        pix[0] = (int32_t)fu;
        pix[1] = (int32_t)fv;
    }
    // step 6
    if (tex || k.keep) {
        xyz[0] = x; xyz[1] = y; xyz[2] = z;
    } else {
        xyz[0] = xyz[1] = xyz[2] = texture_qnan();
    }
    return tex;
}

}  // namespace cd
