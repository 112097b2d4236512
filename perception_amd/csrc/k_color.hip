// k_color.hip - canonical rule C10: the red-object rectangle of every rgb8 image of a batch.
//
// One workgroup of COLOR_BLOCK threads per frame does the whole rule on a BIT-PACKED mask (32 pixels per word, rows padded to
// whole words; bit b of word w of a row = pixel 32 w + b):
//   1. rgb8 -> 8-bit HSV -> red mask (integers only; the sdiv / hdiv tables come from the host, computed in double);
//   2. 9x9 erosion then 9x9 dilation, each as a horizontal pass (shifts with carries across words) and a vertical pass
//      (9 rows), ping-pong between the two halves of the mask buffer;
//   3. 8-connected components by union-find over RUNS (a run = maximal horizontal stretch of set pixels, named by the linear
//      index of its first pixel): labels live in global memory, hooks are atomicMin, so a component's root is its first
//      raster pixel;
//   4. the thread that finds a root follows that component's outer border (Suzuki-Abe through pixel centres) with the
//      shoelace sum and the bounds accumulated on the way - nothing is stored, so there is no border capacity; the walk is
//      bounded by 8 W H steps (every (pixel, direction) pair at most once), and a walk that runs out reports CD_ERR_CAPACITY;
//   5. largest area2, ties to the first raster pixel: one 64-bit LDS atomicMax of (area2 << 32 | ~first).
// A 640 x 480 mask is 9600 words, so both halves (75 KiB) stay in LDS; an image whose two halves exceed COLOR_LDS_WORDS
// runs the same code on a per-frame global-memory buffer (flat pointers: right, not fast).
#include "kernels.hpp"

namespace cd {

namespace {

__device__ __forceinline__ bool red_pixel(int r, int g, int b, const ColorGate& p, const int* tab) {
    const int v = max(r, max(g, b));
    const int diff = v - min(r, min(g, b));
    const int s = (diff * tab[v] + 2048) >> 12;
    const int h0 = (v == r) ? g - b : (v == g) ? b - r + 2 * diff : r - g + 4 * diff;
    int h = (h0 * tab[256 + diff] + 2048) >> 12;   // arithmetic shift
    if (h < 0) h += 180;
    return (h <= p.h_lo_max || h >= p.h_hi_min) && s >= p.s_min && v >= p.v_min;
}

struct Packed {   // a packed mask and its shape
    uint32_t* m;
    int W, H, words;
    __device__ __forceinline__ uint32_t valid(int w) const { return (w == words - 1 && (W & 31)) ? ((1u << (W & 31)) - 1u) : ~0u; }
    // word w of row y; outside the image, and in the pad bits of a row's last word, `fill`
    __device__ __forceinline__ uint32_t rd(int y, int w, uint32_t fill) const {
        if (y < 0 || y >= H || w < 0 || w >= words) return fill;
        return m[(size_t)y * words + w] | (fill & ~valid(w));
    }
    __device__ __forceinline__ bool at(int x, int y) const {
        if (x < 0 || x >= W || y < 0 || y >= H) return false;
        return (m[(size_t)y * words + (x >> 5)] >> (x & 31)) & 1u;
    }
    // linear index of the first pixel of the run that holds the set pixel (x, y)
    __device__ __forceinline__ int run_start(int x, int y) const {
        int w = x >> 5;
        uint32_t z = ~m[(size_t)y * words + w] & ((1u << (x & 31)) - 1u);   // clear pixels left of x in its word
        while (!z) {
            if (--w < 0) return y * W;
            z = ~m[(size_t)y * words + w];
        }
        return y * W + 32 * w + (32 - __clz(z));
    }
};

// one horizontal (9 pixels) or vertical (9 rows) pass of an erosion (fill = ~0: AND) or a dilation (fill = 0: OR)
template <bool ERODE, bool HORIZONTAL>
__device__ __forceinline__ void morph_pass(const Packed& in, uint32_t* out, int tid) {
    const uint32_t fill = ERODE ? ~0u : 0u;
    const int total = in.words * in.H;
    for (int i = tid; i < total; i += COLOR_BLOCK) {
        const int y = i / in.words, w = i - y * in.words;
        uint32_t acc = in.rd(y, w, fill);
        if (HORIZONTAL) {
            const uint32_t c = acc, l = in.rd(y, w - 1, fill), r = in.rd(y, w + 1, fill);
#pragma unroll
            for (int k = 1; k <= 4; ++k) {
                const uint32_t right = (c >> k) | (r << (32 - k));   // bit x = pixel x + k
                const uint32_t left = (c << k) | (l >> (32 - k));    // bit x = pixel x - k
                acc = ERODE ? (acc & right & left) : (acc | right | left);
            }
        } else {
#pragma unroll
            for (int k = 1; k <= 4; ++k) {
                const uint32_t a = in.rd(y - k, w, fill), b = in.rd(y + k, w, fill);
                acc = ERODE ? (acc & a & b) : (acc | a | b);
            }
        }
        out[i] = acc & in.valid(w);
    }
}

__device__ __forceinline__ int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_root(const int* lab, int x) {
    for (int l = ld_label(lab + x); l != x; l = ld_label(lab + x)) x = l;   // labels only ever decrease: finite
    return x;
}

__device__ __forceinline__ void unite(int* lab, int a, int b) {
    for (;;) {
        a = find_root(lab, a);
        b = find_root(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);   // hook the larger root under the smaller
        if (old == a) return;
        a = old;                                  // a had been hooked meanwhile: its old parent still has to meet b
    }
}

__device__ __forceinline__ int dir_dx(int d) { return (int)((0x901Au >> (2 * d)) & 3u) - 1; }   // 1 1 0 -1 -1 -1 0 1
__device__ __forceinline__ int dir_dy(int d) { return (int)((0x01A9u >> (2 * d)) & 3u) - 1; }   // 0 1 1 1 0 -1 -1 -1

}  // namespace

__global__ void __launch_bounds__(COLOR_BLOCK) k_color_bbox(const uint8_t* __restrict__ rgb, int W, int H, ColorGate prm,
                                                            const int* __restrict__ tables, uint32_t* gmask, int* labels,
                                                            size_t label_pitch, ColorRecord* __restrict__ out, int* __restrict__ status) {
    CD_FRONT_PRIO();
    __shared__ uint32_t s_mask[COLOR_LDS_WORDS];
    __shared__ int s_tab[512];
    __shared__ unsigned long long s_best;
    __shared__ int s_ncomp, s_nmask, s_err;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    const int words = (W + 31) >> 5;
    const int MW = words * H;
    uint32_t* A = gmask ? gmask + (size_t)f * 2 * (size_t)MW : s_mask;
    uint32_t* B = A + MW;
    int* lab = labels + (size_t)f * label_pitch;
    const uint8_t* img = rgb + (size_t)f * (size_t)W * H * 3;
    for (int i = tid; i < 512; i += COLOR_BLOCK) s_tab[i] = tables[i];
    if (tid == 0) { s_best = 0ull; s_ncomp = 0; s_nmask = 0; s_err = 0; }
    __syncthreads();

    // ---- 1. mask.  Rows of whole 4-pixel groups on a 4-byte aligned image: 12 bytes = 4 pixels per lane, 8 lanes make a word
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3u) == 0) {
        const int chunks = (W + 255) >> 8;
        for (int it = wave; it < H * chunks; it += COLOR_BLOCK / 64) {
            const int y = it / chunks, c = it - y * chunks;
            const int x = 256 * c + 4 * lane;
            uint32_t nib = 0;
            if (x < W) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(img + ((size_t)y * W + x) * 3);
                const uint32_t a = q[0], b = q[1], d = q[2];   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                nib |= red_pixel(a & 255, (a >> 8) & 255, (a >> 16) & 255, prm, s_tab) ? 1u : 0u;
                nib |= red_pixel(a >> 24, b & 255, (b >> 8) & 255, prm, s_tab) ? 2u : 0u;
                nib |= red_pixel((b >> 16) & 255, b >> 24, d & 255, prm, s_tab) ? 4u : 0u;
                nib |= red_pixel((d >> 8) & 255, (d >> 16) & 255, d >> 24, prm, s_tab) ? 8u : 0u;
            }
            uint32_t v = nib << (4 * (lane & 7));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            const int wi = 8 * c + (lane >> 3);
            if ((lane & 7) == 0 && wi < words) A[(size_t)y * words + wi] = v;
        }
    } else {
        const int chunks = (W + 63) >> 6;
        for (int it = wave; it < H * chunks; it += COLOR_BLOCK / 64) {
            const int y = it / chunks, c = it - y * chunks;
            const int x = 64 * c + lane;
            bool on = false;
            if (x < W) {
                const uint8_t* q = img + ((size_t)y * W + x) * 3;
                on = red_pixel(q[0], q[1], q[2], prm, s_tab);
            }
            const unsigned long long bal = __ballot(on);
            if (lane == 0) {
                A[(size_t)y * words + 2 * c] = (uint32_t)bal;
                if (2 * c + 1 < words) A[(size_t)y * words + 2 * c + 1] = (uint32_t)(bal >> 32);
            }
        }
    }
    __syncthreads();

    // ---- 2. the opening: erosion (outside = set) then dilation (outside = clear), 9 x 9 each
    Packed pa{A, W, H, words}, pb{B, W, H, words};
    morph_pass<true, true>(pa, B, tid);
    __syncthreads();
    morph_pass<true, false>(pb, A, tid);
    __syncthreads();
    morph_pass<false, true>(pa, B, tid);
    __syncthreads();
    morph_pass<false, false>(pb, A, tid);
    __syncthreads();

    // ---- 3. components: every run starts as its own root ...
    int cnt = 0;
    for (int i = tid; i < MW; i += COLOR_BLOCK) {
        const int y = i / words, w = i - y * words;
        const uint32_t cur = A[i];
        cnt += __popc(cur);
        const uint32_t curL = (cur << 1) | (w > 0 ? A[i - 1] >> 31 : 0u);
        for (uint32_t st = cur & ~curL; st; st &= st - 1) {
            const int p = y * W + 32 * w + (__ffs(st) - 1);
            __hip_atomic_store(lab + p, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0 && cnt) atomicAdd(&s_nmask, cnt);
    __syncthreads();
    // ... and meets the runs of the row above that touch it.  Each touching pair (run, upper run) is united at least once:
    // at the pair's leftmost contact, which is a NW contact at a run's first pixel, a N contact whose NW is clear, or a NE
    // contact whose N is clear.
    for (int i = tid + words; i < MW; i += COLOR_BLOCK) {
        const int y = i / words, w = i - y * words;
        const uint32_t cur = A[i];
        if (!cur) continue;
        const uint32_t up = A[i - words];
        const uint32_t curL = (cur << 1) | (w > 0 ? A[i - 1] >> 31 : 0u);
        const uint32_t upL = (up << 1) | (w > 0 ? A[i - words - 1] >> 31 : 0u);
        const uint32_t upR = (up >> 1) | (w + 1 < words ? A[i - words + 1] << 31 : 0u);
        const int x0 = 32 * w;
        for (uint32_t mk = cur & upL & ~curL; mk; mk &= mk - 1) {
            const int x = x0 + __ffs(mk) - 1;
            unite(lab, pa.run_start(x, y), pa.run_start(x - 1, y - 1));
        }
        for (uint32_t mk = cur & up & ~upL; mk; mk &= mk - 1) {
            const int x = x0 + __ffs(mk) - 1;
            unite(lab, pa.run_start(x, y), pa.run_start(x, y - 1));
        }
        for (uint32_t mk = cur & upR & ~up; mk; mk &= mk - 1) {
            const int x = x0 + __ffs(mk) - 1;
            unite(lab, pa.run_start(x, y), pa.run_start(x + 1, y - 1));
        }
    }
    __syncthreads();

    // ---- 4. + 5. every root's outer border, followed by the thread that meets the root
    unsigned long long best = 0ull;
    int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    const long long max_steps = 8ll * W * H;
    for (int i = tid; i < MW; i += COLOR_BLOCK) {
        const int y = i / words, w = i - y * words;
        const uint32_t cur = A[i];
        const uint32_t curL = (cur << 1) | (w > 0 ? A[i - 1] >> 31 : 0u);
        for (uint32_t st = cur & ~curL; st; st &= st - 1) {
            const int sx = 32 * w + (__ffs(st) - 1), sy = y;
            const int p = sy * W + sx;
            if (ld_label(lab + p) != p) continue;
            atomicAdd(&s_ncomp, 1);
            int x0 = sx, x1 = sx, y0 = sy, y1 = sy;
            long long sum = 0;
            int d1 = -1;
            for (int k = 1; k < 8 && d1 < 0; ++k) {   // clockwise from the (clear) west neighbour
                const int d = (4 + k) & 7;
                if (pa.at(sx + dir_dx(d), sy + dir_dy(d))) d1 = d;
            }
            if (d1 >= 0) {
                const int lx = sx + dir_dx(d1), ly = sy + dir_dy(d1);   // the walk's last point
                int cx = sx, cy = sy, dprev = d1;
                long long steps = 0;
                for (;;) {
                    int nx = cx, ny = cy, d = dprev;
                    for (int k = 1; k <= 8; ++k) {   // counter-clockwise, starting after the point the walk came from
                        d = (dprev - k) & 7;
                        nx = cx + dir_dx(d);
                        ny = cy + dir_dy(d);
                        if (pa.at(nx, ny)) break;
                    }
                    sum += (long long)(cx - sx) * (ny - sy) - (long long)(nx - sx) * (cy - sy);   // (relative to the start: same sum)
                    x0 = min(x0, cx); x1 = max(x1, cx); y0 = min(y0, cy); y1 = max(y1, cy);
                    if (nx == sx && ny == sy && cx == lx && cy == ly) break;
                    if (++steps > max_steps) { s_err = 1; break; }
                    cx = nx; cy = ny; dprev = (d + 4) & 7;
                }
            }
            const unsigned long long a2 = (unsigned long long)(sum < 0 ? -sum : sum);
            const unsigned long long key = (a2 << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p);
            if (key > best) { best = key; bx0 = x0; by0 = y0; bx1 = x1; by1 = y1; }
        }
    }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    ColorRecord* o = out + f;
    if (tid == 0) {
        o->n_components = s_ncomp;
        o->n_mask = s_nmask;
        status[f] = s_err ? CD_ERR_CAPACITY : CD_OK;
        if (s_best == 0ull) { o->rect[0] = o->rect[1] = o->rect[2] = o->rect[3] = 0; o->found = 0; o->area2 = 0; }
    }
    if (best && best == s_best) {
        o->rect[0] = bx0 - prm.margin;
        o->rect[1] = by0 - prm.margin;
        o->rect[2] = bx1 + 1 + prm.margin;   // x + w + margin
        o->rect[3] = by1 + 1 + prm.margin;
        o->found = 1;
        o->area2 = (int)(best >> 32);
    }
}

bool color_fits_lds(int W, int H) { return 2ll * ((W + 31) / 32) * (long long)H <= (long long)COLOR_LDS_WORDS; }

void launch_color_bbox(hipStream_t s, const uint8_t* rgb, int W, int H, int F, const ColorGate& prm, const int* tables,
                       uint32_t* gmask, int* labels, size_t label_pitch, ColorRecord* out, int* status) {
    hipLaunchKernelGGL(k_color_bbox, dim3(F), dim3(COLOR_BLOCK), 0, s, rgb, W, H, prm, tables, gmask, labels, label_pitch, out, status);
}

}  // namespace cd
