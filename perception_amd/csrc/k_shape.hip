// k_shape.hip - canonical rule C13 on the device: the principal frame of a point set (cd_shape_frames) and, in
// its fused form, the per-cluster ICP guess of CD_GUESS_CLUSTER.
//
// One 256-thread workgroup per point set.  Pass 1 walks the set's float4 records with a strided loop: nine fixed-point int64
// sums per lane (rule C4: order-free), reduced inside each wave and through LDS.  One lane turns the totals into mean, covariance
// and axes (shape_frame_math.hpp: a fixed Jacobi sequence in explicit round-to-nearest double operations).  Pass 2 projects every
// point on the axes; min and max are exact, so the extents are order-free too.  One lane writes the record and - fused form -
// the guess of rule C13 step 5 against the slot's template record: into guess[16 k] (what k_icp_apply_guess moves the sources by)
// and into Tfinal of both parity states of ICP problem k (final_transformation_ = guess).  No atomics on global memory.
#include "kernels.hpp"
#include "shape_frame_math.hpp"

namespace cd {

__global__ void __launch_bounds__(BLOCK) k_shape_frames(const IcpCluster* __restrict__ cl, const float4* __restrict__ pts,
                                                        ShapeFrame* __restrict__ rec, const ShapeFrame* __restrict__ tframe,
                                                        float* __restrict__ guess, IcpState* __restrict__ st) {
    __shared__ unsigned long long s_sum[WAVES_PER_BLOCK][9];
    __shared__ double s_mm[WAVES_PER_BLOCK][6];
    __shared__ int s_bad[WAVES_PER_BLOCK];
    __shared__ ShapeFrame s_rec;
    const int k = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const IcpCluster c = cl[k];
    const int n = (c.n > 0 && c.n <= SHAPE_N_MAX) ? c.n : 0;   // (a set over the count is refused without being read)
    const float4* __restrict__ P = pts + c.src_off;
    // pass 1: moments
    unsigned long long S[9] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const float4 p = P[i];
        bad = bad || !shape_coord_ok(p.x, p.y, p.z);
        S[0] += (unsigned long long)fixq(p.x, FIX_SHIFT);
        S[1] += (unsigned long long)fixq(p.y, FIX_SHIFT);
        S[2] += (unsigned long long)fixq(p.z, FIX_SHIFT);
        S[3] += (unsigned long long)fixq(__fmul_rn(p.x, p.x), FIX_SHIFT);
        S[4] += (unsigned long long)fixq(__fmul_rn(p.x, p.y), FIX_SHIFT);
        S[5] += (unsigned long long)fixq(__fmul_rn(p.x, p.z), FIX_SHIFT);
        S[6] += (unsigned long long)fixq(__fmul_rn(p.y, p.y), FIX_SHIFT);
        S[7] += (unsigned long long)fixq(__fmul_rn(p.y, p.z), FIX_SHIFT);
        S[8] += (unsigned long long)fixq(__fmul_rn(p.z, p.z), FIX_SHIFT);
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const unsigned long long t = wave_sum_u64(S[j]);
        if (lane == 0) s_sum[w][j] = t;
    }
    const uint64_t any_bad = ballot64(bad);
    if (lane == 0) s_bad[w] = any_bad != 0ull ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int refused = 0;
        for (int q = 0; q < WAVES_PER_BLOCK; ++q) refused |= s_bad[q];
        if (c.n > SHAPE_N_MAX) shape_empty(c.n, SHAPE_ERR_CAPACITY, &s_rec);
        else if (refused) shape_empty(n, SHAPE_ERR_INVALID, &s_rec);
        else if (n < 3) shape_empty(n, SHAPE_ERR_FEW, &s_rec);
        else {
            long long T[9];
            for (int j = 0; j < 9; ++j) {
                unsigned long long t = 0ull;
                for (int q = 0; q < WAVES_PER_BLOCK; ++q) t += s_sum[q][j];
                T[j] = (long long)t;
            }
            shape_empty(n, SHAPE_OK, &s_rec);
            shape_solve(T, n, &s_rec);
        }
    }
    __syncthreads();
    const bool ok = s_rec.status == SHAPE_OK;   // (uniform)
    if (ok) {
        // pass 2: extents along the axes
        double mean[3], A[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) mean[j] = s_rec.mean[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) A[j] = s_rec.axes[j];
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            const float4 p = P[i];
            double q[3];
            shape_project(mean, A, p.x, p.y, p.z, q);
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], q[a]); hi[a] = fmax(hi[a], q[a]); }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo[a] = fmin(lo[a], __shfl_xor(lo[a], o, 64));
                hi[a] = fmax(hi[a], __shfl_xor(hi[a], o, 64));
            }
            if (lane == 0) { s_mm[w][a] = lo[a]; s_mm[w][3 + a] = hi[a]; }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double l = s_mm[0][a], h = s_mm[0][3 + a];
                for (int q = 1; q < WAVES_PER_BLOCK; ++q) { l = fmin(l, s_mm[q][a]); h = fmax(h, s_mm[q][3 + a]); }
                s_rec.lo[a] = rn_dadd(l, 0.0);   // (a zero extent is stored as +0, whichever zero the reduction met first)
                s_rec.hi[a] = rn_dadd(h, 0.0);
            }
        }
        rec[k] = s_rec;
        if (guess) {
            float G[16];
            const int slot = (c.slot >= 0 && c.slot < CD_MAX_TEMPLATES) ? c.slot : 0;
            shape_guess(s_rec, tframe[slot], G);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                guess[16 * (size_t)k + j] = G[j];
                st[2 * (size_t)k].Tfinal[j] = G[j];
                st[2 * (size_t)k + 1].Tfinal[j] = G[j];
            }
        }
    }
}

// Point set k = the n points at pts + cl[k].src_off (cl[k].n of them) -> rec[k].  guess != nullptr (the fused form): tframe holds
// CD_MAX_TEMPLATES template records, guess 16 floats and st two IcpStates per set.
void launch_shape_frames(hipStream_t s, int n_sets, const IcpCluster* cl, const float4* pts, ShapeFrame* rec, const ShapeFrame* tframe,
                         float* guess, IcpState* st) {
    if (n_sets <= 0) return;
    hipLaunchKernelGGL(k_shape_frames, dim3(n_sets), dim3(BLOCK), 0, s, cl, pts, rec, tframe, guess, st);
}

}  // namespace cd
