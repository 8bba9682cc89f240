// fav_corrupt_c.hpp - the ImageNet-C style corruption family behind fav_op_corrupt_c (include/fav.h; DESIGN.md section 2,
// item 5d).  Eight corruptions of uint8 [n][H][W][3] frames into fp32 [n][H][W][3] in [0,1], every one a pure function of
// (seed, global frame index) like corrupt_kernel.  x_c = (float)u8 * (1.0f / 255.0f); the fp32 operations run in the order
// written (the library is built with -ffp-contract=off); the definitions are stated in DESIGN.md and restated for the tests
// in tests/corrupt_c_ref.py.  Included by fav.hip after fav_kernels.hpp (philox4x32_10, u01).
//
//   pointwise (impulse, speckle, brightness, saturate): corrupt_c_point_kernel, four pixels a thread
//   contrast : contrast_kernel, every block of a frame re-reduces that frame's three channel sums (wave butterflies, no atomics)
//   pixelate : pixelate_kernel, one block per row of cells, exact integer sums
//   gaussian blur : gauss_blur_kernel, row pass into LDS and column pass out of it in one launch
//   defocus blur  : defocus_kernel, the fp32 source tile plus halo in LDS, four pixels a thread
#pragma once

namespace fav {

enum { CC_IMPULSE = 0, CC_SPECKLE = 1, CC_GAUSSIAN_BLUR = 2, CC_DEFOCUS_BLUR = 3, CC_CONTRAST = 4, CC_PIXELATE = 5,
       CC_BRIGHTNESS = 6, CC_SATURATE = 7, CC_COUNT = 8 };
constexpr int CC_GAUSS_MAX_R = 32;                       // 65 taps
constexpr int CC_DISK_MAX_R = 14;                        // radius 12 + alias kernel 2: 29 x 29 taps
constexpr int CC_TILE = 32;                              // output tile edge of the two blur kernels
// how the four-pixel kernels store: the shipped way, and the two it was measured against (tools/corrupt_c_bench.py --ab, EXPERIMENTS build)
enum { CC_STORE_STAGED = 0, CC_STORE_FLOAT4 = 1, CC_STORE_SCALAR = 2 };
constexpr int CC_PIXELATE_MAX_W = 2048;                  // 28 bytes of LDS per column

struct CorruptCParams {
    float a, b;
    uint32_t seed_lo, seed_hi;
    long long first_index;
};
struct GaussTaps { float v[2 * CC_GAUSS_MAX_R + 1]; };
struct DiskTaps { float v[(2 * CC_DISK_MAX_R + 1) * (2 * CC_DISK_MAX_R + 1)]; };   // 3364 bytes of the 4 KiB of kernel arguments

// ---- host: the taps the two blur kernels use (also handed out by fav_corruption_taps)
inline int gauss_radius(float sigma) { return (int)(4.0 * (double)sigma + 0.5); }
inline void gauss_taps(float sigma, int R, float* out) {
    double w[2 * CC_GAUSS_MAX_R + 1], sum = 0.0;
    for (int d = -R; d <= R; ++d) {
        const double q = (double)d / (double)sigma;
        sum += w[d + R] = std::exp(-0.5 * q * q);
    }
    for (int i = 0; i <= 2 * R; ++i) out[i] = (float)(w[i] / sum);
}
inline int disk_radius(float a) { const int r = (int)a; return r + (r <= 8 ? 1 : 2); }
// the disk dx^2 + dy^2 <= r^2 on the (2R+1)^2 grid, normalised, smoothed separably (rows, then columns; zero padding) by the
// normalised (2ks+1)-tap Gaussian of sigma b, renormalised to sum 1 in double, rounded to fp32; row-major
inline void disk_taps(float a, float b, float* out) {
    const int r = (int)a, ks = r <= 8 ? 1 : 2, R = r + ks, S = 2 * R + 1;
    constexpr int MAXN = (2 * CC_DISK_MAX_R + 1) * (2 * CC_DISK_MAX_R + 1);
    double disk[MAXN], tmp[MAXN], res[MAXN];       // 20 KB of stack: the launch path allocates nothing
    const int N = S * S;
    for (int i = 0; i < N; ++i) disk[i] = 0.0;
    int cnt = 0;
    for (int y = -R; y <= R; ++y)
        for (int x = -R; x <= R; ++x)
            if (x * x + y * y <= r * r) { disk[(size_t)(y + R) * S + (x + R)] = 1.0; ++cnt; }
    for (int i = 0; i < N; ++i) disk[i] /= (double)cnt;
    double g[5], gs = 0.0;
    for (int k = -ks; k <= ks; ++k) {
        const double q = (double)k / (double)b;
        gs += g[k + ks] = std::exp(-0.5 * q * q);
    }
    for (int k = 0; k <= 2 * ks; ++k) g[k] /= gs;
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            double s = 0.0;
            for (int k = -ks; k <= ks; ++k)
                if (x + k >= 0 && x + k < S) s += g[k + ks] * disk[(size_t)y * S + (x + k)];
            tmp[(size_t)y * S + x] = s;
        }
    double total = 0.0;
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            double s = 0.0;
            for (int k = -ks; k <= ks; ++k)
                if (y + k >= 0 && y + k < S) s += g[k + ks] * tmp[(size_t)(y + k) * S + x];
            total += res[(size_t)y * S + x] = s;
        }
    for (int i = 0; i < N; ++i) out[i] = (float)(res[i] / total);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---- groups of four pixels.  A run of cnt pixels starts at byte address `in`, a = in & 3: pixel p sits at in + 3p, which is
// 4-byte aligned exactly when p = a (mod 4).  Group 0 is the a pixels in front of the first aligned one, group g >= 1 the four
// pixels from a + 4(g - 1) on (fewer at the end of the run): a full group is three aligned dwords in and 48 bytes out.
struct PxGroup {
    long long p0;
    int k;
};
__device__ __forceinline__ PxGroup px_group(int a, long long g, long long cnt) {
    PxGroup r;
    if (g == 0) {
        r.p0 = 0;
        r.k = (int)((long long)a < cnt ? a : cnt);
    } else {
        r.p0 = a + 4 * (g - 1);
        const long long left = cnt - r.p0;
        r.k = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    }
    return r;
}
inline long long px_group_count(long long cnt) { return 1 + (cnt + 3) / 4; }   // an upper bound for every a
// the three float4 stores of a full group need out + 3 (a + 4m) sixteen-byte aligned
__device__ __forceinline__ bool px_vec_out(const float* out, int a) { return ((uintptr_t)(out + 3 * a) & 15) == 0; }

// f(b0, b1, b2, v): one pixel's three bytes -> its three output values; called for the group's pixels in order
template <class F>
__device__ __forceinline__ void px_group_values(const uint8_t* in, const PxGroup g, F f, float (&v)[12]) {
    const uint8_t* p = in + 3 * g.p0;
    if (g.k == 4) {
        const uint32_t* q = (const uint32_t*)p;
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        f(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, v);
        f(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, v + 3);
        f((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, v + 6);
        f((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, v + 9);
        return;
    }
    for (int j = 0; j < g.k; ++j) f((uint32_t)p[3 * j], (uint32_t)p[3 * j + 1], (uint32_t)p[3 * j + 2], v + 3 * j);
}
// a group's values straight to memory: three float4 stores at a 48-byte lane stride, or scalar stores
__device__ __forceinline__ void px_store_group(float* out, const PxGroup g, bool vec_out, const float (&v)[12]) {
    float* o = out + 3 * g.p0;
    if (g.k == 4 && vec_out) {
        float4* o4 = (float4*)o;
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
        return;
    }
    for (int i = 0; i < 3 * g.k; ++i) o[i] = v[i];
}
// 256 full groups, one a thread, in group order: every wave turns its 64 x 48 bytes round in LDS so that each of its three
// store instructions writes 1 KiB of consecutive bytes: 20 - 26 % faster than float4 stores at a 48-byte lane stride for impulse
// and brightness in a same-process A/B (profiles/corrupt_c_bench.txt).  Every thread of the block calls it; `out` is where the first group's values go, 16-byte aligned.
__device__ __forceinline__ void px_store_chunk(float* out, float4* stage, const float (&v)[12]) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    float4* s = stage + w * 192;
    s[3 * l] = make_float4(v[0], v[1], v[2], v[3]);
    s[3 * l + 1] = make_float4(v[4], v[5], v[6], v[7]);
    s[3 * l + 2] = make_float4(v[8], v[9], v[10], v[11]);
    __syncthreads();
    float4* o = (float4*)out + w * 192;
    o[l] = s[l]; o[64 + l] = s[64 + l]; o[128 + l] = s[128 + l];
    __syncthreads();
}
// A run's groups in chunks of 256, one chunk a block at a time.  Position i of chunk c is aligned group 1 + 256 c + i; the
// head (group 0) takes the position behind the last aligned group.  A chunk of 256 full groups goes out through
// px_store_chunk; f(grp) returns the pixel function of one group.
template <class F>
__device__ __forceinline__ void px_run_chunk(const uint8_t* in, float* out, int a, long long cnt, long long chunk, bool vec_out,
                                             bool staged, float4* stage, F f) {
    const long long groups = 1 + (cnt + 3) / 4;
    const long long idx = chunk * 256 + threadIdx.x;
    PxGroup grp;
    grp.p0 = 0; grp.k = 0;
    if (idx + 1 < groups) grp = px_group(a, idx + 1, cnt);
    else if (idx + 1 == groups) grp = px_group(a, 0, cnt);
    float v[12];
    if (grp.k) px_group_values(in, grp, f(grp), v);
    const long long first = a + 4 * (chunk * 256);                    // the chunk's first pixel
    if (staged && vec_out && first + 1024 <= cnt) px_store_chunk(out + 3 * first, stage, v);
    else if (grp.k) px_store_group(out, grp, vec_out, v);
}
__host__ __device__ inline long long px_chunk_count(long long cnt) { return (1 + (cnt + 3) / 4 + 255) / 256; }

// ---- the pointwise kinds.  Philox counter = (pixel index in the frame, low 32 bits of first_index + f, stream, 0);
// stream 16 = impulse, 17 = speckle (corrupt_kernel holds 0, 2, 3, 4 and 7).
template <int KIND>
__device__ __forceinline__ void point_pixel(const CorruptCParams& cp, uint32_t px, uint32_t frame, uint32_t b0, uint32_t b1,
                                            uint32_t b2, float* o) {
    const float x0 = (float)b0 * (1.0f / 255.0f), x1 = (float)b1 * (1.0f / 255.0f), x2 = (float)b2 * (1.0f / 255.0f);
    if constexpr (KIND == CC_IMPULSE) {
        // channel c is hit iff u01(word c) < a; a hit is 1 if bit c of word 3 is set, else 0
        const uint4 u = philox4x32_10(make_uint4(px, frame, 16u, 0u), cp.seed_lo, cp.seed_hi);
        o[0] = u01(u.x) < cp.a ? ((u.w & 1u) ? 1.0f : 0.0f) : x0;
        o[1] = u01(u.y) < cp.a ? ((u.w & 2u) ? 1.0f : 0.0f) : x1;
        o[2] = u01(u.z) < cp.a ? ((u.w & 4u) ? 1.0f : 0.0f) : x2;
    } else if constexpr (KIND == CC_SPECKLE) {
        // Box-Muller as corrupt_kernel's Gaussian mode forms n0, n1, n2
        const uint4 a = philox4x32_10(make_uint4(px, frame, 17u, 0u), cp.seed_lo, cp.seed_hi);
        const float r0 = sqrtf(-2.0f * logf(1.0f - u01(a.x))), r1 = sqrtf(-2.0f * logf(1.0f - u01(a.z)));
        const float t0 = 6.2831853071795864f * u01(a.y), t1 = 6.2831853071795864f * u01(a.w);
        const float z0 = r0 * cosf(t0), z1 = r0 * sinf(t0), z2 = r1 * cosf(t1);
        o[0] = clamp01(x0 + (x0 * cp.a) * z0);
        o[1] = clamp01(x1 + (x1 * cp.a) * z1);
        o[2] = clamp01(x2 + (x2 * cp.a) * z2);
    } else if constexpr (KIND == CC_BRIGHTNESS) {
        // HSV value shift V -> min(V + a, 1) at fixed hue and saturation: every channel scales by V2 / V
        const float V = fmaxf(fmaxf(x0, x1), x2);
        const float V2 = fminf(V + cp.a, 1.0f);
        if (V == 0.0f) {
            o[0] = V2; o[1] = V2; o[2] = V2;
        } else {
            const float s = V2 / V;
            o[0] = fminf(x0 * s, 1.0f); o[1] = fminf(x1 * s, 1.0f); o[2] = fminf(x2 * s, 1.0f);
        }
    } else {
        // HSV saturation S -> clamp(S a + b) at fixed hue and value; grey has hue 0 (k = 0, 1, 1)
        const float V = fmaxf(fmaxf(x0, x1), x2), m = fminf(fminf(x0, x1), x2);
        const float S = V > 0.0f ? (V - m) / V : 0.0f;
        const float S2 = clamp01(S * cp.a + cp.b);
        const bool col = V > m;
        const float k0 = col ? (V - x0) / (V - m) : 0.0f;
        const float k1 = col ? (V - x1) / (V - m) : 1.0f;
        const float k2 = col ? (V - x2) / (V - m) : 1.0f;
        o[0] = clamp01(V * (1.0f - S2 * k0));
        o[1] = clamp01(V * (1.0f - S2 * k1));
        o[2] = clamp01(V * (1.0f - S2 * k2));
    }
}

// 3 bytes in and 12 bytes out per pixel are what limits it: a thread takes four pixels, 12 bytes in as three dwords and three
// float4 stores out, turned round in LDS so that a wave's stores are consecutive.  The call's n * H * W pixels are one run.
template <int KIND>
__global__ __launch_bounds__(256) void corrupt_c_point_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                              long long npx, long long total, CorruptCParams cp, int store_mode) {
    __shared__ float4 stage[768];
    const int a = (int)((uintptr_t)in & 3);
    const bool vec_out = store_mode != CC_STORE_SCALAR && px_vec_out(out, a);
    const long long chunks = px_chunk_count(total);
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)
        px_run_chunk(in, out, a, total, chunk, vec_out, store_mode == CC_STORE_STAGED, stage, [&](const PxGroup grp) {
            const long long f0 = grp.p0 / npx;
            return [&cp, npx, f = f0, px = grp.p0 - f0 * npx](uint32_t b0, uint32_t b1, uint32_t b2, float* v) mutable {
                point_pixel<KIND>(cp, (uint32_t)px, (uint32_t)(cp.first_index + f), b0, b1, b2, v);
                if (++px == npx) { px = 0; ++f; }
            };
        });
}

// ---- contrast: out = clamp((x - m_c) a + m_c), m_c = (float)((double)S_c / ((double)H W 255)), S_c the exact integer sum of
// channel c over the frame.  `per_frame` blocks share a frame; each of them reduces the whole frame itself (at most a few
// hundred KB, served by the L2 after the first block) - per-thread integer sums, a 64-lane butterfly, four wave totals through
// LDS - and then writes its share of the frame's groups.  No atomics, no second launch, no buffer.
__global__ __launch_bounds__(256) void contrast_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long long npx,
                                                       int per_frame, double den, float ca, int store_mode) {
    __shared__ unsigned long long wave_sum[4][3];
    __shared__ float4 stage[768];
    const long long f = blockIdx.x / per_frame;
    const int part = (int)(blockIdx.x - f * per_frame);
    const uint8_t* fin = in + (size_t)f * npx * 3;
    float* fout = out + (size_t)f * npx * 3;
    const int a = (int)((uintptr_t)fin & 3);
    const long long groups = 1 + (npx + 3) / 4;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (long long g = threadIdx.x; g < groups; g += 256) {
        const PxGroup grp = px_group(a, g, npx);
        const uint8_t* p = fin + 3 * grp.p0;
        if (grp.k == 4) {
            const uint32_t* q = (const uint32_t*)p;
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
            s0 += (w0 & 255u) + (w0 >> 24) + ((w1 >> 16) & 255u) + ((w2 >> 8) & 255u);
            s1 += ((w0 >> 8) & 255u) + (w1 & 255u) + (w1 >> 24) + ((w2 >> 16) & 255u);
            s2 += ((w0 >> 16) & 255u) + ((w1 >> 8) & 255u) + (w2 & 255u) + (w2 >> 24);
        } else {
            for (int j = 0; j < grp.k; ++j) { s0 += p[3 * j]; s1 += p[3 * j + 1]; s2 += p[3 * j + 2]; }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_sum[threadIdx.x >> 6][0] = s0; wave_sum[threadIdx.x >> 6][1] = s1; wave_sum[threadIdx.x >> 6][2] = s2;
    }
    __syncthreads();
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long S = wave_sum[0][c] + wave_sum[1][c] + wave_sum[2][c] + wave_sum[3][c];
        m[c] = (float)((double)S / den);
    }
    const bool vec_out = store_mode != CC_STORE_SCALAR && px_vec_out(fout, a);
    const long long chunks = px_chunk_count(npx);
    for (long long chunk = part; chunk < chunks; chunk += per_frame)
        px_run_chunk(fin, fout, a, npx, chunk, vec_out, store_mode == CC_STORE_STAGED, stage, [&](const PxGroup) {
            return [m0 = m[0], m1 = m[1], m2 = m[2], ca](uint32_t b0, uint32_t b1, uint32_t b2, float* v) {
                v[0] = clamp01(((float)b0 * (1.0f / 255.0f) - m0) * ca + m0);
                v[1] = clamp01(((float)b1 * (1.0f / 255.0f) - m1) * ca + m1);
                v[2] = clamp01(((float)b2 * (1.0f / 255.0f) - m2) * ca + m2);
            };
        });
}

// ---- pixelate: the frame is cut into hd x wd cells, source pixel (y, x) belongs to cell (((2y+1) hd) / (2H), ((2x+1) wd) / (2W));
// every pixel of a cell becomes (float)sum_c / (float)(count * 255), sum_c the exact integer sum of the cell.  One block per
// row of cells: byte-column sums over the cell row's source rows (coalesced byte loads), then one thread per cell, then the
// cell row's output rows.  LDS: colsum u32[3W], cellof u32[W], cellval f32[3 wd].
__device__ __forceinline__ long long cell_start(long long c, long long cells, long long size) {
    // the first index i with ((2i+1) cells) / (2 size) >= c
    const long long num = 2 * size * c - cells;
    return num <= 0 ? 0 : (num + 2 * cells - 1) / (2 * cells);
}
__global__ __launch_bounds__(256) void pixelate_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int H, int W,
                                                       int hd, int wd, long long items) {
    extern __shared__ uint32_t pix_lds[];
    uint32_t* colsum = pix_lds;
    uint32_t* cellof = pix_lds + 3 * W;
    float* cellval = (float*)(pix_lds + 4 * W);
    const int W3 = 3 * W;
    for (int x = threadIdx.x; x < W; x += 256) cellof[x] = ((2u * (uint32_t)x + 1u) * (uint32_t)wd) / (2u * (uint32_t)W);
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long f = item / hd;
        const long long cy = item - f * hd;
        const long long y0 = cell_start(cy, hd, H), y1 = cell_start(cy + 1, hd, H);
        const uint8_t* fin = in + ((size_t)f * H + (size_t)y0) * W3;
        float* fout = out + ((size_t)f * H + (size_t)y0) * W3;
        const int rows = (int)(y1 - y0);
        for (int j = threadIdx.x; j < W3; j += 256) {
            uint32_t s = 0;
            for (int r = 0; r < rows; ++r) s += fin[(size_t)r * W3 + j];
            colsum[j] = s;
        }
        __syncthreads();
        for (int cx = threadIdx.x; cx < wd; cx += 256) {
            const int xa = (int)cell_start(cx, wd, W), xb = (int)cell_start(cx + 1, wd, W);
            unsigned long long s0 = 0, s1 = 0, s2 = 0;
            for (int x = xa; x < xb; ++x) { s0 += colsum[3 * x]; s1 += colsum[3 * x + 1]; s2 += colsum[3 * x + 2]; }
            const float den = (float)((unsigned long long)rows * (unsigned long long)(xb - xa) * 255ull);
            cellval[3 * cx] = (float)s0 / den; cellval[3 * cx + 1] = (float)s1 / den; cellval[3 * cx + 2] = (float)s2 / den;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            for (int j = threadIdx.x; j < W3; j += 256) {
                const int x = j / 3, c = j - 3 * x;
                fout[(size_t)r * W3 + j] = cellval[3 * cellof[x] + c];
            }
        __syncthreads();
    }
}

// ---- the sliding window both blur kernels run on: four neighbouring outputs o_i = sum_t tap(t) * e(i + t), t ascending, each
// e of C values.  Element t + 3 is loaded once at step t and used by four outputs from registers; the loop is unrolled by
// four so that the window's rotation is a renaming, not a move.
template <int C, class Tap, class Load>
__device__ __forceinline__ void slide4(int ntaps, Tap tap, Load load, float (&acc)[4 * C]) {
    float w[4][C];
    load(0, w[0]); load(1, w[1]); load(2, w[2]);
    for (int t0 = 0; t0 < ntaps; t0 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + k;
            if (t < ntaps) {
                load(t + 3, w[(k + 3) & 3]);
                const float tp = tap(t);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[i * C + c] += tp * w[(k + i) & 3][c];
            }
        }
    }
}

struct BlurTile {
    long long f;
    int x0, y0;
};
__device__ __forceinline__ BlurTile blur_tile(long long t, int tiles_x, int tiles_y) {
    const long long rest = t / tiles_x;
    BlurTile b;
    b.x0 = (int)(t - rest * tiles_x) * CC_TILE;
    b.f = rest / tiles_y;
    b.y0 = (int)(rest - b.f * tiles_y) * CC_TILE;
    return b;
}

// ---- gaussian blur, both passes in one launch.  Per 32 x 32 output tile: the uint8 source tile plus halo (replicate borders:
// the index is clamped) goes to LDS; the row pass writes fp32 into LDS for the tile's rows +- R; the column pass reads that
// with the same taps and stores clamp(result).  LDS at R = 24: 80 x 97 x 4 + 80 x 80 x 3 = 50 KB; at R = 32: 63.4 KB.
constexpr int CC_MID_LD = CC_TILE * 3 + 1;               // 97: the row pass writes 12 floats a lane, four rows a half-wave
inline size_t gauss_blur_lds(int R) {
    const size_t T = CC_TILE + 2 * R;
    return T * CC_MID_LD * 4 + T * T * 3;
}
__global__ __launch_bounds__(256) void gauss_blur_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int H, int W,
                                                         int R, GaussTaps tp, int tiles_x, int tiles_y, long long tiles) {
    extern __shared__ __align__(16) unsigned char blur_lds[];
    const int T = CC_TILE + 2 * R, ntaps = 2 * R + 1, TW3 = T * 3;
    float* mid = (float*)blur_lds;                       // [T][CC_MID_LD]
    uint8_t* src = blur_lds + (size_t)T * CC_MID_LD * 4; // [T][T * 3]
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const BlurTile b = blur_tile(t, tiles_x, tiles_y);
        const uint8_t* fin = in + (size_t)b.f * H * W * 3;
        float* fout = out + (size_t)b.f * H * W * 3;
        for (int r = threadIdx.x >> 6; r < T; r += 4) {
            const int y = min(max(b.y0 - R + r, 0), H - 1);
            for (int j = threadIdx.x & 63; j < TW3; j += 64) {
                const int col = j / 3, c = j - 3 * col;
                const int x = min(max(b.x0 - R + col, 0), W - 1);
                src[r * TW3 + j] = fin[((size_t)y * W + x) * 3 + c];
            }
        }
        __syncthreads();
        for (int it = threadIdx.x; it < T * 8; it += 256) {           // row r, pixels 4g .. 4g + 3
            const int r = it >> 3, g = it & 7;
            const uint8_t* s = src + r * TW3 + g * 12;
            float acc[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            slide4<3>(ntaps, [&](int k) { return tp.v[k]; },
                      [&](int p, float* v) {
                          v[0] = (float)s[3 * p] * (1.0f / 255.0f);
                          v[1] = (float)s[3 * p + 1] * (1.0f / 255.0f);
                          v[2] = (float)s[3 * p + 2] * (1.0f / 255.0f);
                      }, acc);
            float* m = mid + r * CC_MID_LD + g * 12;
#pragma unroll
            for (int i = 0; i < 12; ++i) m[i] = acc[i];
        }
        __syncthreads();
        for (int it = threadIdx.x; it < 8 * CC_TILE * 3; it += 256) { // rows 4rg .. 4rg + 3 of value j = 3 column + channel
            const int rg = it / (CC_TILE * 3), j = it - rg * (CC_TILE * 3);
            const float* m = mid + (rg * 4) * CC_MID_LD + j;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            slide4<1>(ntaps, [&](int k) { return tp.v[k]; }, [&](int p, float* v) { v[0] = m[p * CC_MID_LD]; }, acc);
            const int x = b.x0 + j / 3;
            if (x < W) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int y = b.y0 + rg * 4 + i;
                    if (y < H) fout[((size_t)y * W + b.x0) * 3 + j] = clamp01(acc[i]);
                }
            }
        }
        __syncthreads();
    }
}

// ---- defocus blur: a (2R+1)^2 disk, borders reflect-101 (period 2(n-1), any distance; a dimension of 1 maps to 0).  The
// source tile plus halo is staged in LDS as fp32 x_c; a thread owns four neighbouring pixels of one output row and slides
// the window along every tap row, so a staged value is read once per tap row and used four times.  The row stride is odd:
// a half-wave is eight groups of four rows, 12 g + stride * row then falls on 32 different banks.  LDS at R = 12: 37.9 KB.
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}
inline int defocus_ld(int R) { return ((CC_TILE + 2 * R) * 3) | 1; }
inline size_t defocus_lds(int R) { return (size_t)(CC_TILE + 2 * R) * defocus_ld(R) * 4; }
__global__ __launch_bounds__(256) void defocus_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int H, int W, int R,
                                                      DiskTaps tp, int tiles_x, int tiles_y, long long tiles) {
    extern __shared__ __align__(16) unsigned char blur_lds[];
    float* tile = (float*)blur_lds;
    const int T = CC_TILE + 2 * R, ntaps = 2 * R + 1, TW3 = T * 3, LD = TW3 | 1;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const BlurTile b = blur_tile(t, tiles_x, tiles_y);
        const uint8_t* fin = in + (size_t)b.f * H * W * 3;
        float* fout = out + (size_t)b.f * H * W * 3;
        for (int r = threadIdx.x >> 6; r < T; r += 4) {
            const int y = reflect101(b.y0 - R + r, H);
            for (int j = threadIdx.x & 63; j < TW3; j += 64) {
                const int col = j / 3, c = j - 3 * col;
                const int x = reflect101(b.x0 - R + col, W);
                tile[r * LD + j] = (float)fin[((size_t)y * W + x) * 3 + c] * (1.0f / 255.0f);
            }
        }
        __syncthreads();
        const int g = threadIdx.x & 7, r = threadIdx.x >> 3;          // output row r, pixels 4g .. 4g + 3
        float acc[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int dy = 0; dy < ntaps; ++dy) {
            const float* s = tile + (r + dy) * LD + g * 12;
            const int base = dy * ntaps;
            slide4<3>(ntaps, [&](int k) { return tp.v[base + k]; },
                      [&](int p, float* v) { v[0] = s[3 * p]; v[1] = s[3 * p + 1]; v[2] = s[3 * p + 2]; }, acc);
        }
        const int y = b.y0 + r;
        if (y < H) {
            float* o = fout + ((size_t)y * W + b.x0 + 4 * g) * 3;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (b.x0 + 4 * g + i < W) {
                    o[3 * i] = clamp01(acc[3 * i]); o[3 * i + 1] = clamp01(acc[3 * i + 1]); o[3 * i + 2] = clamp01(acc[3 * i + 2]);
                }
        }
        __syncthreads();
    }
}

}  // namespace fav
