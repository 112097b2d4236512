// allpairs_scan.hpp - the exact all-pairs scan of k_pair_score (rule C21) and k_icp_recip_flags (rule C22), written once: a
// workgroup of THREADS threads holds a range of queries in registers, up to ROWS per lane, and passes ALL the targets through LDS
// in tiles; the loop reads target e for all lanes at once - one address, a broadcast ds_read_b128, no bank conflict - and hands
// dist2(query, target) of every live row to the kernel's own update (three subtractions, three products, two sums per pair).
// The pieces, in the order a kernel uses them:
//   scan_row / scan_clamp   which query a lane's row j holds: a row beyond the range holds a copy of the range's last query (its
//                           loads stay inside the range, the kernel ignores what it finds);
//   scan_load_tile          cnt targets into the tile, as they are or under a 4 x 4 matrix, padded with +inf points to a multiple
//                           of 8 - what the loop is unrolled by; an +inf point is at distance +inf or NaN from everything and
//                           never enters a minimum;
//   scan_tile_rows          the loop, instantiated per number of live rows so that a range's empty rows cost nothing.
// The constants (rows, tile, threads) and the update are the kernel's.  A query's result is complete inside one workgroup and
// the updates are minima: nothing depends on the order of the targets or on how the queries are split.
#pragma once
#include "common.hpp"

namespace cd {

// row j of this thread is query scan_row(j) of the workgroup's range (counted from the range's first), live while below the
// range's qn >= 1 queries; scan_clamp: the query a row loads
template <int THREADS>
__device__ __forceinline__ int scan_row(int j) { return j * THREADS + (int)threadIdx.x; }
__device__ __forceinline__ int scan_clamp(int r, int qn) { return r < qn ? r : qn - 1; }
template <int THREADS>
__device__ __forceinline__ int scan_live_rows(int qn) { return (qn + THREADS - 1) / THREADS; }

// targets gp[t0 .. t0 + cnt) -> tile[0 .. cnt8), cnt8 = cnt rounded up to a multiple of 8 (returned).  A target is stored as it
// is; a kernel with MOVED targets says per call whether these are (as_is), or go under the row-major 4 x 4 matrix T (xform_row,
// evaluated here, once per load).  The whole workgroup calls it, and a barrier follows.  The tile holds at least cnt8 points.
template <int THREADS, bool MOVED = false>
__device__ __forceinline__ int scan_load_tile(float4* tile, const float4* gp, int t0, int cnt, bool as_is = true, const float* T = nullptr) {
    const int cnt8 = (cnt + 7) & ~7;
    for (int e = (int)threadIdx.x; e < cnt8; e += THREADS) {
        float4 g = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        if (e < cnt) {
            const float4 p = gp[t0 + e];
            if (!MOVED || as_is) g = make_float4(p.x, p.y, p.z, 0.f);
            else g = make_float4(xform_row(T, 0, p.x, p.y, p.z), xform_row(T, 1, p.x, p.y, p.z), xform_row(T, 2, p.x, p.y, p.z), 0.f);
        }
        tile[e] = g;
    }
    return cnt8;
}

// One tile against the lane's first LIVE rows: up(j, e, d) with d = dist2(query of row j, target e of the tile)
template <int LIVE, int ROWS, class Update>
__device__ __forceinline__ void scan_tile(const float4* __restrict__ tile, int cnt8, const float (&qx)[ROWS], const float (&qy)[ROWS],
                                          const float (&qz)[ROWS], Update up) {
#pragma unroll 8
    for (int e = 0; e < cnt8; ++e) {
        const float4 g = tile[e];   // (the same address in every lane)
#pragma unroll
        for (int j = 0; j < LIVE; ++j) up(j, e, dist2(qx[j], qy[j], qz[j], g.x, g.y, g.z));
    }
}
// ... for `rows` live rows, 1 <= rows <= ROWS <= 4
template <int ROWS, class Update>
__device__ __forceinline__ void scan_tile_rows(int rows, const float4* __restrict__ tile, int cnt8, const float (&qx)[ROWS], const float (&qy)[ROWS],
                                               const float (&qz)[ROWS], Update up) {
    static_assert(ROWS >= 1 && ROWS <= 4, "one instantiation per number of live rows");
    switch (rows) {   // (a case that ROWS rules out falls through to the last one)
        case 1: if constexpr (ROWS > 1) { scan_tile<1, ROWS>(tile, cnt8, qx, qy, qz, up); break; }
        case 2: if constexpr (ROWS > 2) { scan_tile<2, ROWS>(tile, cnt8, qx, qy, qz, up); break; }
        case 3: if constexpr (ROWS > 3) { scan_tile<3, ROWS>(tile, cnt8, qx, qy, qz, up); break; }
        default: scan_tile<ROWS, ROWS>(tile, cnt8, qx, qy, qz, up);
    }
}

}  // namespace cd
