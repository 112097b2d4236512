// k_box_fit.hip - canonical rule C24 (perception_amd/box_fit.py is the specification, box_fit_math.hpp the
// arithmetic): the box fit of clusters, opt-in through cd_set_box_fit, and the kernel behind cd_box_fit_points.
//
// One workgroup of four waves takes cluster items from the launch's queue - the host has sorted them largest first and has put the
// frame's oriented plane and metric basis (steps 1 and 2, host arithmetic) into the item.  Per item:
//   1. quantise   every point is range-checked (step 10) and, for a cluster of at most BOX_LDS_POINTS points, its (qh, u, v) go to
//                 LDS.  A larger cluster is quantised again from global memory wherever a pass below reads a point: the same
//                 integers, since box_quantise is a fixed sequence of rounded operations.
//   2. select     the k-th largest qh exactly: four rounds over the biased integer, 8-bit digits from the top, each counting its
//                 digit in a 256-bin LDS histogram; wave 0 finds the bin the rank falls into (k_icp_reject's selection, from above).
//   3. top        n_top, the int64 sum of the top set's qh and its lexicographically smallest (u, v) - the hull's first vertex - as
//                 the minimum of a 64-bit integer key: order-free.
//   4. march      k_prism's: one workgroup-wide reduction per hull vertex with the exact int64 comparator (prism_better) over the
//                 top set; it stops at the first vertex, at a set that is one point, or at vertex PRISM_MAX_HULL + 1 (overflow).
//                 No pruning pass before it and no compaction of the top set: a cluster is a few thousand points, not a table's
//                 tens of thousands of inliers, and its hull a few dozen vertices.  The cost is points x hull vertices - beyond
//                 the LDS cap with a point's 27 double operations each time; profiles/EXPERIMENTS.md has the worst case measured.
//   5. edges      the hull sits in LDS; lane t owns the edges t, t + 256, ... and walks all vertices for each (box_edge); the
//                 winner is the workgroup minimum over (area bits, edge) - non-negative doubles order like their bits.  The
//                 shoelace terms are summed as integers on the way.
//   6. record     the lane that owns the winning edge still holds its extents: it runs box_finish - rn_* operations only, no
//                 contraction - and writes the record with ordinary vector stores.
// Integer sums, minima and counts only: nothing depends on how points fall to lanes, waves or workgroups.  No atomic on floating
// point anywhere.
// Bounds: a point index is below the item's n (the host guarantees src_off + n inside the point buffer); the LDS arrays are
// indexed by it only when n <= BOX_LDS_POINTS; a hull slot is written only below PRISM_MAX_HULL; a histogram bin is a byte.
#include <climits>

#include "kernels.hpp"
#include "box_fit_math.hpp"

namespace cd {

static_assert(BLOCK == 256, "one histogram bin per thread when it is cleared");

__global__ void __launch_bounds__(BLOCK) k_box_fit(int nitems, const BoxItem* __restrict__ items, const float4* __restrict__ pts, cd_box_fit* __restrict__ out,
                                                   int* __restrict__ queue) {
    __shared__ int32_t s_qh[BOX_LDS_POINTS], s_u[BOX_LDS_POINTS], s_v[BOX_LDS_POINTS];
    __shared__ int32_t s_hull[2 * PRISM_MAX_HULL];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[2];
    __shared__ PrismPoint s_best[2][WAVES_PER_BLOCK];
    __shared__ int s_valid[2][WAVES_PER_BLOCK];
    __shared__ int s_cnt[WAVES_PER_BLOCK];
    __shared__ unsigned long long s_sum[WAVES_PER_BLOCK];
    __shared__ long long s_start[WAVES_PER_BLOCK];
    __shared__ unsigned long long s_area[WAVES_PER_BLOCK];
    __shared__ int s_edge[WAVES_PER_BLOCK];
    __shared__ unsigned long long s_shoe;
    __shared__ int s_item, s_bad;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (;;) {
        if (tid == 0) { s_item = atomicAdd(queue, 1); s_bad = 0; s_shoe = 0ull; }
        __syncthreads();
        const int it = __builtin_amdgcn_readfirstlane(s_item);
        if (it >= nitems) return;   // (the whole workgroup)
        do {
            const BoxItem* __restrict__ I = items + it;
            const int n = __builtin_amdgcn_readfirstlane(I->n), src_off = __builtin_amdgcn_readfirstlane(I->src_off);
            const int32_t band_q = __builtin_amdgcn_readfirstlane(I->band_q);
            cd_box_fit* __restrict__ R = out + __builtin_amdgcn_readfirstlane(I->rec);
            if (n < 3) {
                if (tid == 0) box_empty(n, 0, 0, CD_ERR_FEW_CORRESPONDENCES, 0, R);
                break;
            }
            const BoxBasis B = I->B;
            const float4* __restrict__ P = pts + src_off;
            const bool in_lds = n <= BOX_LDS_POINTS;

            // ---- 1: the range check; (qh, u, v) to LDS when they fit
            bool bad = false;
            for (int i = tid; i < n; i += BLOCK) {
                const float4 p = P[i];
                bad = bad || !box_coord_ok(p.x, p.y, p.z);
                if (in_lds) box_quantise(B, p.x, p.y, p.z, &s_qh[i], &s_u[i], &s_v[i]);
            }
            if (bad) atomicOr(&s_bad, 1);
            __syncthreads();
            if (s_bad || !B.have) {
                if (tid == 0) box_empty(n, 0, 0, s_bad ? CD_ERR_INVALID_ARG : CD_ERR_NO_MODEL, 0, R);
                break;
            }
            auto height_of = [&](int i) -> int32_t {
                if (in_lds) return s_qh[i];
                const float4 p = P[i];
                return prism_quantise(rn_dadd(box_dot(B.nrm, (double)p.x, (double)p.y, (double)p.z), B.dd));
            };
            auto point_of = [&](int i, int32_t* qh, PrismPoint* q) {
                if (in_lds) { *qh = s_qh[i]; q->u = s_u[i]; q->v = s_v[i]; return; }
                const float4 p = P[i];
                box_quantise(B, p.x, p.y, p.z, qh, &q->u, &q->v);
            };

            // ---- 2: the k-th largest qh
            uint32_t prefix = 0u;
            uint32_t rank = 1u + (uint32_t)(n >> 6);
            for (int r = 0; r < 4; ++r) {
                const int shift = 24 - 8 * r;
                const uint32_t settled = ~(0xffffffffu >> (8 * r));   // the digits the earlier rounds fixed: none in round 0
                s_hist[tid] = 0u;
                __syncthreads();
                for (int i = tid; i < n; i += BLOCK) {
                    const uint32_t key = box_key(height_of(i));
                    if ((key & settled) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                if (w == 0) {   // lane l owns the bins 4 l .. 4 l + 3; `above`: the counted keys in the bins of the lanes to its right
                    const uint32_t h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
                    const uint32_t tot = h0 + h1 + h2 + h3;
                    uint32_t incl = tot;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const uint32_t t = __shfl_down(incl, o, WAVE);
                        if (lane + o < 64) incl += t;
                    }
                    const uint32_t above = incl - tot;
                    if (rank > above && rank <= incl) {   // one lane: the counted keys are at least `rank` (it is at most n, and shrinks with them)
                        uint32_t left = rank - above, d = 3u;
                        if (left > h3) { left -= h3; d = 2u; if (left > h2) { left -= h2; d = 1u; if (left > h1) { left -= h1; d = 0u; } } }
                        s_sel[0] = 4u * (uint32_t)lane + d;
                        s_sel[1] = left;
                    }
                }
                __syncthreads();
                prefix |= s_sel[0] << shift;
                rank = s_sel[1];
            }
            const int32_t href = (int32_t)(prefix ^ 0x80000000u);
            const int32_t thr = href - band_q;   // (|href| <= 2^29, band_q < 2^23)

            // ---- 3: the top set's count, sum and first vertex
            int cnt = 0;
            unsigned long long qs = 0ull;
            long long first = LLONG_MAX;
            for (int i = tid; i < n; i += BLOCK) {
                int32_t qh;
                PrismPoint q;
                point_of(i, &qh, &q);
                if (qh >= thr) {
                    ++cnt;
                    qs += (unsigned long long)(long long)qh;
                    first = min(first, (long long)q.u * 4294967296ll + ((long long)q.v + 2147483648ll));
                }
            }
            cnt = wave_sum_i32(cnt);
            qs = wave_sum_u64(qs);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, WAVE));
            if (lane == 0) { s_cnt[w] = cnt; s_sum[w] = qs; s_start[w] = first; }
            __syncthreads();
            int n_top = 0;
            unsigned long long qsum = 0ull;
            first = LLONG_MAX;
            for (int q = 0; q < WAVES_PER_BLOCK; ++q) { n_top += s_cnt[q]; qsum += s_sum[q]; first = min(first, s_start[q]); }
            // (href itself is in the top set: n_top >= 1 and `first` is a point)

            // ---- 4: the march (k_prism.hip, C) over the top set
            PrismPoint cur;
            cur.u = (int32_t)(first >> 32);
            cur.v = (int32_t)((long long)(first & 0xffffffffll) - 2147483648ll);
            const PrismPoint start = cur;
            if (tid == 0) { s_hull[0] = cur.u; s_hull[1] = cur.v; }
            int nh = 1, overflow = 0;
            for (int step = 0; step <= PRISM_MAX_HULL; ++step) {
                PrismPoint best = {0, 0};
                bool valid = false;
                for (int j = tid; j < n; j += BLOCK) {
                    int32_t qh;
                    PrismPoint q;
                    point_of(j, &qh, &q);
                    if (qh < thr || (q.u == cur.u && q.v == cur.v)) continue;
                    if (!valid || prism_better(cur, best, q)) { best = q; valid = true; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    PrismPoint q;
                    q.u = __shfl_xor(best.u, o, WAVE);
                    q.v = __shfl_xor(best.v, o, WAVE);
                    const bool qvalid = __shfl_xor((int)valid, o, WAVE) != 0;
                    if (qvalid && (!valid || prism_better(cur, best, q))) { best = q; valid = true; }
                }
                const int buf = step & 1;   // (two buffers: one barrier per vertex)
                if (lane == 0) { s_best[buf][w] = best; s_valid[buf][w] = valid ? 1 : 0; }
                __syncthreads();
                valid = false;
                for (int q = 0; q < WAVES_PER_BLOCK; ++q) {
                    const PrismPoint c = s_best[buf][q];
                    if (s_valid[buf][q] && (!valid || prism_better(cur, best, c))) { best = c; valid = true; }
                }
                if (!valid || (best.u == start.u && best.v == start.v)) break;   // all points are one; or the hull is closed
                if (nh == PRISM_MAX_HULL) { overflow = 1; break; }
                if (tid == 0) { s_hull[2 * nh] = best.u; s_hull[2 * nh + 1] = best.v; }
                ++nh;
                cur = best;
            }
            if (overflow || nh < 3) {
                if (tid == 0) box_empty(n, n_top, overflow ? 0 : nh, overflow ? CD_ERR_CAPACITY : CD_ERR_NO_MODEL, overflow, R);
                break;
            }
            __syncthreads();   // (the hull is whole)

            // ---- 5: every edge's rectangle; the smallest area, then the lowest edge
            unsigned long long my_bits = ~0ull;
            int my_edge = INT_MAX;
            BoxEdge my_E = {0, 0, 0, 0, 0, 0.0};
            unsigned long long shoe = 0ull;
            for (int i = tid; i < nh; i += BLOCK) {
                const BoxEdge E = box_edge(s_hull, nh, i);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(E.area);
                if (bits < my_bits) { my_bits = bits; my_edge = i; my_E = E; }   // (i ascends: a tie keeps the lower edge)
                shoe += (unsigned long long)box_shoelace_term(s_hull, nh, i);
            }
            unsigned long long bb = my_bits;
            int be = my_edge;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long ob = __shfl_xor(bb, o, WAVE);
                const int oe = __shfl_xor(be, o, WAVE);
                if (ob < bb || (ob == bb && oe < be)) { bb = ob; be = oe; }
            }
            shoe = wave_sum_u64(shoe);
            if (lane == 0) { s_area[w] = bb; s_edge[w] = be; atomicAdd(&s_shoe, shoe); }
            __syncthreads();
            bb = s_area[0]; be = s_edge[0];
            for (int q = 1; q < WAVES_PER_BLOCK; ++q) {
                const unsigned long long ob = s_area[q];
                const int oe = s_edge[q];
                if (ob < bb || (ob == bb && oe < be)) { bb = ob; be = oe; }
            }

            // ---- 6: the record, by the lane that owns the winning edge
            if (my_edge == be) box_finish(B, n, n_top, href, (int64_t)qsum, s_hull, nh, be, my_E, (int64_t)s_shoe, R);
        } while (false);
        __syncthreads();   // (s_item, s_bad, s_shoe and the hull are rewritten at the top)
    }
}

void launch_box_fit(hipStream_t s, int nitems, int n_wg, const BoxItem* items, const float4* pts, cd_box_fit* out, int* queue) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_box_fit, dim3(std::max(1, std::min(nitems, n_wg))), dim3(BLOCK), 0, s, nitems, items, pts, out, queue);
}

}  // namespace cd
