// k_labels.hip - canonical rule C15: the label of every input record (pixel) of the last fused call, by provenance.
//
// Three steps on the context's stream, inside the label calls only (labels.hip):
//   1. k_label_voxel_keys     the frame's sorted keys (one per run or per point, whichever path the voxel stage took) compacted to
//                             one key per voxel, in the order of d_vox: voxel v's key is the v-th distinct key;
//   2. k_label_voxel_classes  voxel v's class: CD_LABEL_GATED, then CD_LABEL_PLANE for every entry of the call's plane index list,
//                             then - for the voxels that the S3 predicate (extract_flags.hpp, what k_extract_scatter applied)
//                             moved into the object cloud, numbered by an order-preserving scan - CD_LABEL_OBJECT or
//                             CD_LABEL_CLUSTER0 + r from the call's cluster labels; after a call that filtered its object
//                             clouds (rule C16) that number goes through the filter's map first: a voxel the filter removed
//                             stays CD_LABEL_GATED;
//   3. k_label_points         the batch as ONE linear stream of records or pixels (as k_deproject takes it): the S0 predicate, the
//                             point's key in the form step 1 found, a binary search among the frame's voxel keys (at most 32
//                             probes, ~15 on a 640 x 480 frame: the table of a frame is ~70 KB and stays in L2; neighbouring
//                             pixels probe neighbouring lines), the class of the voxel found.  Four labels per lane, their four
//                             searches in step (four probes in flight per round), one dword store where the output is 4-byte
//                             aligned.
// One workgroup per frame in steps 1 and 2: their running counts are carried in order, no atomics, no chained scan.  Every loop is
// bounded by a count clamped to the row it indexes, and every index read from memory is range-checked before it is used.
#include <algorithm>

#include "extract_flags.hpp"
#include "kernels.hpp"
#include "label_math.hpp"
#include "outlier_math.hpp"

namespace cd {

// ---- step 1 ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_label_voxel_keys(const uint32_t* __restrict__ keys, int N, const FrameState* __restrict__ fs,
                                                            int by_runs, uint32_t* __restrict__ vkey, int vpitch) {
    __shared__ int s_cnt[WAVES_PER_BLOCK];
    const int f = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(max(by_runs ? fs[f].n_runs : fs[f].n_c, 0), N);
    const int nv = min(max(fs[f].n_v, 0), vpitch);
    const uint32_t* k = keys + (size_t)f * N;
    uint32_t* o = vkey + (size_t)f * vpitch;
    const uint64_t lt = lanemask_lt();
    int out0 = 0;
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int base = t0 + w * WAVE_SPAN + lane;
        uint32_t cur[ITEMS], left[ITEMS];
        uint64_t bal[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {   // (clamped indices: all loads of the wave's rows in flight together)
            const int e = base + j * WAVE;
            cur[j] = k[max(min(e, n - 1), 0)];
            left[j] = k[max(min(e - 1, n - 1), 0)];
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int e = base + j * WAVE;
            bal[j] = __ballot(e < n && (e == 0 || cur[j] != left[j]));
        }
        int tot;
        int pos = out0 + tile_prefix<ITEMS>(bal, s_cnt, &tot);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int r = pos + __popcll(bal[j] & lt);
            if (((bal[j] >> lane) & 1ull) && r < nv) o[r] = cur[j];
            pos += __popcll(bal[j]);
        }
        out0 += tot;
    }
}

// ---- step 2 ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_label_voxel_classes(const float4* __restrict__ vox, int N, const FrameState* __restrict__ fs,
                                                               const float4* __restrict__ model, const int* __restrict__ have, float thr,
                                                               int negative, int crop2, float z2lo, float z2hi, BBoxGate gate, FrameRects rects,
                                                               const int* __restrict__ plane_idx, const int* __restrict__ label,
                                                               uint8_t* __restrict__ vclass, int vpitch, OutlierMap omap) {
    __shared__ int s_cnt[WAVES_PER_BLOCK];
    const int f = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nv = min(min(max(fs[f].n_v, 0), vpitch), N);
    const int n_plane = min(max(fs[f].n_plane, 0), N), n_o = min(max(fs[f].n_o, 0), N);
    // what S3 moved: the object cloud itself, or - a filtered call - the cloud the filter read, whose row of the map holds one entry each
    const int n_s3 = omap.map ? min(min(max(omap.rec[f].n_before, 0), omap.pitch), N) : n_o;
    const int* omap_row = omap.map ? omap.map + (size_t)f * omap.pitch : nullptr;
    const size_t fbase = (size_t)f * N;
    uint8_t* cls = vclass + (size_t)f * vpitch;
    for (int v = threadIdx.x; v < nv; v += BLOCK) cls[v] = (uint8_t)LABEL_GATED;
    __syncthreads();
    for (int i = threadIdx.x; i < n_plane; i += BLOCK) {
        const int v = plane_idx[fbase + i];
        if (v >= 0 && v < nv) cls[v] = (uint8_t)LABEL_PLANE;
    }
    __syncthreads();
    if (n_s3 <= 0 || n_o <= 0) return;   // (the frame's chain ended before S3, or S3 - or the filter - kept nothing)
    frame_rect(gate, rects, f);
    const float4 m = model[f];
    const int hv = have[f];
    const float4* P = vox + fbase;
    const uint64_t lt = lanemask_lt();
    int out0 = 0;
    for (int t0 = 0; t0 < nv; t0 += TILE) {
        const int base = t0 + w * WAVE_SPAN + lane;
        float4 p[ITEMS];
        uint64_t bal[ITEMS];
        load_rows_clamped<ITEMS>(P, base, nv, p);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            bool inl = false, obj = false;
            if (base + j * WAVE < nv) extract_flags(m, hv, thr, negative, crop2, z2lo, z2hi, gate, p[j], inl, obj);
            bal[j] = __ballot(obj);
        }
        int tot;
        int pos = out0 + tile_prefix<ITEMS>(bal, s_cnt, &tot);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int v = base + j * WAVE;
            int r = pos + __popcll(bal[j] & lt);   // (r: the voxel's place among what S3 moved)
            const bool moved = ((bal[j] >> lane) & 1ull) && r < n_s3;
            if (moved && omap_row) r = omap_row[r];   // (its place in the object cloud, -1: the filter removed it)
            if (moved && r >= 0 && r < n_o) cls[v] = label_of_rank(label[fbase + r]);
            pos += __popcll(bal[j]);
        }
        out0 += tot;
    }
}

// ---- step 3 ------------------------------------------------------------------------------------------------------------------
struct LabelFrame { LabelGrid g; int nv; };
__device__ __forceinline__ LabelFrame label_frame(const FrameState* __restrict__ fs, int f, int vpitch) {
    LabelFrame L;
    const FrameState& s = fs[f];
    for (int a = 0; a < 3; ++a) { L.g.min_b[a] = s.min_b[a]; L.g.div_b[a] = s.div_b[a]; }
    L.nv = min(max(s.n_v, 0), vpitch);
    return L;
}

constexpr int LBL_PER_LANE = 4;
template <bool DEPTH>
__global__ void __launch_bounds__(BLOCK) k_label_points(const char* __restrict__ rec, size_t stride, const uint16_t* __restrict__ depth,
                                                        LabelPointsParams lp, const FrameState* __restrict__ fs,
                                                        const uint32_t* __restrict__ vkey, const uint8_t* __restrict__ vclass,
                                                        uint8_t* __restrict__ out) {
    const size_t total = (size_t)lp.P * (size_t)lp.F;
    const bool out_vec = (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const bool d_vec = DEPTH && (reinterpret_cast<uintptr_t>(depth) & 7u) == 0;
    const bool r_vec = !DEPTH && stride == 16 && (reinterpret_cast<uintptr_t>(rec) & 15u) == 0;
    for (size_t g0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * LBL_PER_LANE; g0 < total; g0 += (size_t)gridDim.x * BLOCK * LBL_PER_LANE) {
        const int cnt = total - g0 < (size_t)LBL_PER_LANE ? (int)(total - g0) : LBL_PER_LANE;
        // ---- the lane's four records: xyz
        float x[LBL_PER_LANE], y[LBL_PER_LANE], z[LBL_PER_LANE];
        int f = (int)(g0 / lp.P);
        uint32_t p = (uint32_t)(g0 - (size_t)f * lp.P);
        const int f0 = f;
        if (DEPTH) {
            uint32_t d[LBL_PER_LANE] = {0u, 0u, 0u, 0u};
            if (cnt == LBL_PER_LANE && d_vec) {
                const uint2 q = *reinterpret_cast<const uint2*>(depth + g0);
                d[0] = q.x & 0xffffu; d[1] = q.x >> 16; d[2] = q.y & 0xffffu; d[3] = q.y >> 16;
            } else {
                for (int k = 0; k < cnt; ++k) d[k] = depth[g0 + k];
            }
            uint32_t pp = p;
#pragma unroll
            for (int k = 0; k < LBL_PER_LANE; ++k) {
                const uint32_t v = pp / lp.width, u = pp - v * lp.width;
                deproject_c7(u, v, d[k], lp.fx, lp.fy, lp.cx, lp.cy, lp.depth_scale, &x[k], &y[k], &z[k]);
                if (++pp == lp.P) pp = 0;
            }
        } else if (cnt == LBL_PER_LANE && r_vec) {
            float4 q[LBL_PER_LANE];
#pragma unroll
            for (int k = 0; k < LBL_PER_LANE; ++k) q[k] = *reinterpret_cast<const float4*>(rec + (g0 + k) * 16);
#pragma unroll
            for (int k = 0; k < LBL_PER_LANE; ++k) { x[k] = q[k].x; y[k] = q[k].y; z[k] = q[k].z; }
        } else {
#pragma unroll
            for (int k = 0; k < LBL_PER_LANE; ++k) {
                const char* r = rec + (g0 + (size_t)min(k, cnt - 1)) * stride;
                x[k] = *reinterpret_cast<const float*>(r);
                y[k] = *reinterpret_cast<const float*>(r + 4);
                z[k] = *reinterpret_cast<const float*>(r + 8);
            }
        }
        // ---- their labels; the frame's constants are read once per lane and again only where the four records cross a frame
        LabelFrame L = label_frame(fs, f, lp.vpitch);
        uint32_t lab[LBL_PER_LANE], key[LBL_PER_LANE];
        const uint32_t* vk[LBL_PER_LANE];
        const uint8_t* vc[LBL_PER_LANE];
        int nv[LBL_PER_LANE], at[LBL_PER_LANE];
#pragma unroll
        for (int k = 0; k < LBL_PER_LANE; ++k) {
            if (f != f0 && p == 0u && f < lp.F) L = label_frame(fs, f, lp.vpitch);
            const int fk = f < lp.F ? f : f0;                 // (past the batch's end: k >= cnt, nothing is searched)
            vk[k] = vkey + (size_t)fk * lp.vpitch;            // (a frame's row holds vpitch >= 64 words: word 0 is always readable)
            vc[k] = vclass + (size_t)fk * lp.vpitch;
            nv[k] = 0;
            key[k] = 0u;
            uint32_t l = (uint32_t)LABEL_INVALID;
            if (k < cnt && label_finite(x[k], y[k], z[k])) {
                l = (uint32_t)LABEL_CROPPED;
                if (label_kept(x[k], z[k], lp.lim)) {
                    l = (uint32_t)LABEL_GATED;
                    const bool in_grid = L.nv > 0 && (lp.packed ? label_key_packed(x[k], y[k], z[k], lp.inv_leaf, lp.kp, &key[k])
                                                                : label_key_idx(x[k], y[k], z[k], lp.inv_leaf, L.g, &key[k]));
                    if (in_grid) nv[k] = L.nv;
                }
            }
            lab[k] = l;
            if (++p == lp.P) { p = 0u; ++f; }
        }
        // the four searches in step (label_math.hpp), then the classes of the voxels found
        label_lower_bound_n<LBL_PER_LANE>(vk, nv, key, at);
#pragma unroll
        for (int k = 0; k < LBL_PER_LANE; ++k)
            if (at[k] < nv[k] && vk[k][at[k]] == key[k]) lab[k] = vc[k][at[k]];
        if (cnt == LBL_PER_LANE && out_vec) {
            *reinterpret_cast<uint32_t*>(out + g0) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        } else {
            for (int k = 0; k < cnt; ++k) out[g0 + k] = (uint8_t)lab[k];
        }
    }
}

// ---- tint ----------------------------------------------------------------------------------------------------------------------
// four pixels (12 colour bytes, 4 labels) per lane; whole groups move as dwords where both pointers allow it
__global__ void __launch_bounds__(BLOCK) k_tint_labels(uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels, size_t pixels, LabelPalette pal) {
    __shared__ uint32_t s_pal[256];
    s_pal[threadIdx.x] = pal.rgba[threadIdx.x];
    static_assert(BLOCK == 256, "one palette entry per thread");
    __syncthreads();
    const bool vec = (reinterpret_cast<uintptr_t>(rgb) & 3u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3u) == 0;
    for (size_t g0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 4; g0 < pixels; g0 += (size_t)gridDim.x * BLOCK * 4) {
        const int cnt = pixels - g0 < 4 ? (int)(pixels - g0) : 4;
        uint8_t c[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, l[4] = {0, 0, 0, 0};
        if (cnt == 4 && vec) {
            const uint32_t lw = *reinterpret_cast<const uint32_t*>(labels + g0);
            const uint32_t* src = reinterpret_cast<const uint32_t*>(rgb + g0 * 3);
            const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
            for (int k = 0; k < 4; ++k) { l[k] = (uint8_t)(lw >> (8 * k)); c[k] = (uint8_t)(w0 >> (8 * k)); c[4 + k] = (uint8_t)(w1 >> (8 * k)); c[8 + k] = (uint8_t)(w2 >> (8 * k)); }
        } else {
            for (int k = 0; k < cnt; ++k) { l[k] = labels[g0 + k]; for (int q = 0; q < 3; ++q) c[3 * k + q] = rgb[(g0 + k) * 3 + q]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = s_pal[l[k]], a = e >> 24;
#pragma unroll
            for (int q = 0; q < 3; ++q) c[3 * k + q] = label_tint(c[3 * k + q], (e >> (8 * q)) & 0xffu, a);
        }
        if (cnt == 4 && vec) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(rgb + g0 * 3);
            for (int q = 0; q < 3; ++q) dst[q] = (uint32_t)c[4 * q] | ((uint32_t)c[4 * q + 1] << 8) | ((uint32_t)c[4 * q + 2] << 16) | ((uint32_t)c[4 * q + 3] << 24);
        } else {
            for (int k = 0; k < cnt; ++k) for (int q = 0; q < 3; ++q) rgb[(g0 + k) * 3 + q] = c[3 * k + q];
        }
    }
}

// ---- host launchers --------------------------------------------------------------------------------------------------------------
void launch_label_voxel_keys(hipStream_t s, const uint32_t* keys, int N, int F, const FrameState* fs, int by_runs, uint32_t* vkey, int vpitch) {
    hipLaunchKernelGGL(k_label_voxel_keys, dim3(F), dim3(BLOCK), 0, s, keys, N, fs, by_runs, vkey, vpitch);
}
void launch_label_voxel_classes(hipStream_t s, const float4* vox, int N, int F, const FrameState* fs, const float4* model, const int* have,
                                float thr, int negative, int crop2, float z2lo, float z2hi, const BBoxGate& gate, const FrameRects& rects,
                                const int* plane_idx, const int* label, uint8_t* vclass, int vpitch, const OutlierMap& omap) {
    hipLaunchKernelGGL(k_label_voxel_classes, dim3(F), dim3(BLOCK), 0, s, vox, N, fs, model, have, thr, negative, crop2, z2lo, z2hi, gate, rects,
                       plane_idx, label, vclass, vpitch, omap);
}
static unsigned stream_grid(size_t elements) {
    const size_t groups = (elements + (size_t)BLOCK * 4 - 1) / ((size_t)BLOCK * 4);
    return (unsigned)std::max<size_t>(1, std::min<size_t>(groups, 8192));   // grid-stride beyond 32 workgroups per CU
}
void launch_label_points(hipStream_t s, const void* records, size_t stride, const uint16_t* depth, const LabelPointsParams& lp,
                         const FrameState* fs, const uint32_t* vkey, const uint8_t* vclass, uint8_t* out) {
    const size_t total = (size_t)lp.P * (size_t)lp.F;
    if (total == 0) return;
    if (depth)
        hipLaunchKernelGGL(k_label_points<true>, dim3(stream_grid(total)), dim3(BLOCK), 0, s, (const char*)nullptr, (size_t)0, depth, lp, fs, vkey, vclass, out);
    else
        hipLaunchKernelGGL(k_label_points<false>, dim3(stream_grid(total)), dim3(BLOCK), 0, s, (const char*)records, stride, (const uint16_t*)nullptr, lp, fs, vkey, vclass, out);
}
void launch_tint_labels(hipStream_t s, uint8_t* rgb, const uint8_t* labels, size_t pixels, const LabelPalette& pal) {
    if (pixels == 0) return;
    hipLaunchKernelGGL(k_tint_labels, dim3(stream_grid(pixels)), dim3(BLOCK), 0, s, rgb, labels, pixels, pal);
}

}  // namespace cd
