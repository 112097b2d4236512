// extract_flags.hpp - the S3 predicate of one voxel: inlier of the refined plane, member of the object cloud (S3 + S3b + the bbox
// gate).  Shared by the kernels of k_plane.hip that build the plane index list and the object cloud, and by the voxel classes of
// rule C15 (k_labels.hip), which must flag exactly the voxels that k_extract_scatter moved.
#pragma once
#include "kernels.hpp"

namespace cd {
#ifdef __HIPCC__
__device__ __forceinline__ bool plane_inlier(const float4& m, int have, float thr, const float4& p) {
    return have && plane_dist(m.x, m.y, m.z, m.w, p.x, p.y, p.z) < thr;
}

// bbox_filter.cpp:30-51: projection accumulated in double, stored to float, float division, strict compares
__device__ __forceinline__ bool within_bbox(const BBoxGate& g, float x, float y, float z) {
    float u = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(g.P[0], (double)x), __dmul_rn(g.P[1], (double)y)), __dmul_rn(g.P[2], (double)z)), g.P[3]);
    float v = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(g.P[4], (double)x), __dmul_rn(g.P[5], (double)y)), __dmul_rn(g.P[6], (double)z)), g.P[7]);
    const float w = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(g.P[8], (double)x), __dmul_rn(g.P[9], (double)y)), __dmul_rn(g.P[10], (double)z)), g.P[11]);
    u = __fdiv_rn(u, w);
    v = __fdiv_rn(v, w);
    return (g.rect[0] < u && u < g.rect[2]) && (g.rect[1] < v && v < g.rect[3]);
}

// the rectangle of frame f when the gate's rectangles come per frame (CD_BBOX_PER_FRAME / CD_BBOX_COLOR)
__device__ __forceinline__ void frame_rect(BBoxGate& g, const FrameRects& fr, int f) {
    if (!fr.rect) return;
    const int32_t* r = fr.rect + (size_t)f * fr.pitch;
    for (int i = 0; i < 4; ++i) g.rect[i] = (float)r[i];
}

__device__ __forceinline__ void extract_flags(const float4& m, int have, float thr, int negative, int crop2, float z2lo,
                                              float z2hi, const BBoxGate& g, const float4& p, bool& inl, bool& obj) {
    if (g.enable == 2) {   // cd_bbox_filter: the index output is the set of points inside the rectangle
        inl = within_bbox(g, p.x, p.y, p.z);
        obj = false;
        return;
    }
    inl = plane_inlier(m, have, thr, p);
    obj = negative ? !inl : inl;
    if (obj && crop2) obj = (p.z >= z2lo) && (p.z <= z2hi);   // voxel centroids are finite
    if (obj && g.enable) obj = within_bbox(g, p.x, p.y, p.z);
}
#endif
}  // namespace cd
