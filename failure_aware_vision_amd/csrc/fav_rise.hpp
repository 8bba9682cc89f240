// fav_rise.hpp - RISE saliency behind fav_op_rise_mask, fav_op_rise_accumulate and fav_set_rise / fav_classify_rise
// (include/fav.h; Petsiuk et al. 2018).  The classifier is a black box: the frames are classified
// under N random smooth masks, every mask is weighted by the probability the class got under it, and the weighted masks are
// summed.  No tap, no backward pass, any arch.  The mask is a pure integer function of (seed, frame index, mask index, pixel):
// a (g+1) x (g+1) grid of Philox bits, shifted by a Philox draw and upsampled bilinearly in integers to mq in [0, 256], so a
// numpy restatement (tests/rise_ref.py) gives its bits.  Two kernels, one launch each:
//   rise_mask_kernel        the bandwidth kernel, occlude_kernel's shape: four neighbouring pixels a work item, the source
//                           group loaded once and blended and stored once a mask; the grid rows and the shift of the block's
//                           (frame, mask) pairs are drawn by the block into LDS, RISE_MASK_CHUNK masks at a time
//   rise_accumulate_kernel  a block a frame, a thread up to four cells: the mask values are derived again at each cell's sample
//                           pixel from draws staged in LDS (no frame is read), the chains run in mask order, one lane scans
//                           the map for the record
// Included by fav.hip after fav_curve.hpp (curve_frame_error, curve_map_error, curve_fill_error, vpx_fill, map_record_no_class;
// the curve head is this head's twin on the host: perturb_clear .. classify_perturb_head in fav.hip), fav_views.hpp,
// fav_corrupt_c.hpp (px_group), fav_mapbox.hpp (map_box_scan, map_record_store) and fav_kernels.hpp (philox4x32_10, FastDiv).
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int RISE_MAX_MASKS = 8192;
constexpr int RISE_MAX_GRID = 15;              // g + 1 <= 16: a grid row is 16 bits, the grid at most 256 cells = 16 Philox calls
constexpr uint32_t RISE_SITE = 0x715Eu;        // the fourth counter word of every draw
constexpr uint32_t RISE_SHIFT_CHUNK = 16u;     // the first counter word of the shift's draw, behind the grid's 0 .. 15
constexpr int RISE_MASK_CHUNK = 8;             // masks whose draws a block of the mask kernel stages at once
constexpr int RISE_ACC_CHUNK = 32;             // the same for the accumulate head
constexpr int RISE_ACC_THREADS = 256;

// ---- host: the one place the ranges live
inline int rise_cell(int size, int g) { return (size + g - 1) / g; }      // ch = ceil(H / g), cw = ceil(W / g)

// fav_check_rise: the descriptor for H x W frames of `layout`
inline std::string rise_desc_error(const fav_rise* d, int H, int W, int layout) {
    if (!d) return "desc is NULL";
    if (d->struct_size != sizeof(fav_rise)) return "struct_size is not sizeof(fav_rise)";
    if (d->n_masks < 1 || d->n_masks > RISE_MAX_MASKS) return fmt("n_masks=%d outside [1, %d]", d->n_masks, RISE_MAX_MASKS);
    if (d->grid < 1 || d->grid > RISE_MAX_GRID) return fmt("grid=%d outside [1, %d]", d->grid, RISE_MAX_GRID);
    if (d->keep < 1 || d->keep > 255) return fmt("keep=%d outside [1, 255]", d->keep);
    std::string why = curve_frame_error(H, W, layout);
    if (!why.empty()) return why;
    if (d->grid > std::min(H, W)) return fmt("grid=%d above min(H, W)=%d", d->grid, std::min(H, W));
    // the kernels divide 256 * num2 + 2 ch cw <= 1026 ch cw by a launch constant in 32 bits, exact below 2^31
    const long long cells = (long long)rise_cell(H, d->grid) * rise_cell(W, d->grid);
    if (1026 * cells >= (1ll << 31))
        return fmt("frame size %dx%d with grid=%d: 1026 * ceil(H / grid) * ceil(W / grid) reaches 2^31, the mask's 32-bit arithmetic", H, W, d->grid);
    if (layout == FAV_LAYOUT_NHWC_U8) why = curve_fill_error(d->fill_u8, layout);
    return why;
}
// the map of the accumulate head against the frame: every cell holds a pixel
inline std::string rise_map_error(int mh, int mw, int H, int W) {
    std::string why = curve_map_error(mh, mw);
    if (why.empty() && (mh > H || mw > W)) why = fmt("map %dx%d is finer than the %dx%d frame", mh, mw, H, W);
    return why;
}

// ---- the mask function of a launch
struct RiseArg {
    uint32_t seed_lo, seed_hi;
    uint32_t first;            // the low 32 bits of first_image_index
    int g, keep;
    uint32_t ch, cw, ch2, cw2; // ch2 = 2 ch, cw2 = 2 cw
    uint32_t half;             // 2 ch cw
    FastDiv div_ch2, div_cw2, div_q;     // / 2 ch, / 2 cw, / 4 ch cw
};
inline RiseArg rise_arg(const fav_rise& d, long long first_index, int H, int W) {
    RiseArg ra;
    memset(&ra, 0, sizeof ra);
    ra.seed_lo = (uint32_t)d.seed; ra.seed_hi = (uint32_t)(d.seed >> 32);
    ra.first = (uint32_t)(unsigned long long)first_index;
    ra.g = d.grid; ra.keep = d.keep;
    ra.ch = (uint32_t)rise_cell(H, d.grid); ra.cw = (uint32_t)rise_cell(W, d.grid);
    ra.ch2 = 2 * ra.ch; ra.cw2 = 2 * ra.cw;
    ra.half = 2 * ra.ch * ra.cw;
    ra.div_ch2 = fastdiv_make(ra.ch2); ra.div_cw2 = fastdiv_make(ra.cw2); ra.div_q = fastdiv_make(2 * ra.half);
    return ra;
}

// byte j (0 .. 15) of a draw: the dropout reference's order, x's low byte first
__device__ __forceinline__ uint32_t rise_byte(const uint4& u, int j) {
    const int q = j >> 2;
    const uint32_t w = q == 0 ? u.x : (q == 1 ? u.y : (q == 2 ? u.z : u.w));
    return (w >> (8 * (j & 3))) & 0xFFu;
}

// The draws of `count` masks from m_first on, for frame index F, by the threads of a block: rows[ms][gy] holds grid row gy of
// mask m_first + ms, bit gx = cell (gy, gx) is ON; shift[ms] = (dy, dx).  A thread takes a grid row (at most two Philox calls:
// a row of at most 16 cells lies in at most two chunks of 16) or a shift.  The caller puts barriers around it.
__device__ __forceinline__ void rise_stage(const RiseArg& ra, uint32_t F, int m_first, int count, uint32_t (*rows)[16], int2* shift,
                                           int tid, int nthreads) {
    const int per = ra.g + 2;                  // g + 1 rows and the shift
    for (int t = tid; t < count * per; t += nthreads) {
        const int ms = t / per, r = t - ms * per;
        const uint32_t m = (uint32_t)(m_first + ms);
        if (r == ra.g + 1) {
            const uint4 u = philox4x32_10(make_uint4(RISE_SHIFT_CHUNK, F, m, RISE_SITE), ra.seed_lo, ra.seed_hi);
            shift[ms] = make_int2((int)__umulhi(u.x, ra.ch), (int)__umulhi(u.y, ra.cw));
            continue;
        }
        const int j0 = r * (ra.g + 1);
        uint32_t bits = 0;
        int have = -1;
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        for (int gx = 0; gx <= ra.g; ++gx) {
            const int j = j0 + gx;
            if ((j >> 4) != have) {
                have = j >> 4;
                u = philox4x32_10(make_uint4((uint32_t)have, F, m, RISE_SITE), ra.seed_lo, ra.seed_hi);
            }
            bits |= (rise_byte(u, j & 15) < (uint32_t)ra.keep ? 1u : 0u) << gx;
        }
        rows[ms][r] = bits;
    }
}

// One axis of the bilinear upsampling: the two grid lines around shifted pixel p = y + dy (or x + dx) and the weight f of the
// second, in units of 1 / (2 c)
struct RiseAxis {
    uint32_t i0, i1, f;
};
__device__ __forceinline__ RiseAxis rise_axis(int p, uint32_t c, uint32_t c2, const FastDiv& div_c2, int g) {
    const uint32_t num = (uint32_t)max(2 * p + 1 - (int)c, 0);
    RiseAxis a;
    a.i0 = fastdiv(num, div_c2);
    a.f = num - a.i0 * c2;
    if (a.i0 >= (uint32_t)g) { a.i0 = (uint32_t)g; a.f = 0; }
    a.i1 = min(a.i0 + 1u, (uint32_t)g);
    return a;
}
// mq in [0, 256] from the grid rows r0 = rows[ay.i0] and r1 = rows[ay.i1]
__device__ __forceinline__ uint32_t rise_mq(const RiseArg& ra, uint32_t r0, uint32_t r1, const RiseAxis& ay, const RiseAxis& ax) {
    const uint32_t w0 = ra.cw2 - ax.f, w1 = ax.f;
    const uint32_t top = (((r0 >> ax.i0) & 1u) ? w0 : 0u) + (((r0 >> ax.i1) & 1u) ? w1 : 0u);
    const uint32_t bot = (((r1 >> ax.i0) & 1u) ? w0 : 0u) + (((r1 >> ax.i1) & 1u) ? w1 : 0u);
    const uint32_t num2 = (ra.ch2 - ay.f) * top + ay.f * bot;
    return fastdiv(256u * num2 + ra.half, ra.div_q);
}

// ---- the blend.  u8: the three bytes of a pixel in one word - channels 0 and 2 share a multiplication, a 16-bit lane each
// (255 * 256 + 128 < 2^16: no carry leaves a lane).  f32: mq == 256 copies the source bits, mq == 0 stores the fill's, otherwise
// f + w * (p - f), every operation rounded on its own.
__device__ __forceinline__ ViewPx<uint8_t> rise_blend(const ViewPx<uint8_t> p, const ViewPx<uint8_t> f, uint32_t mq) {
    const uint32_t nq = 256u - mq;
    const uint32_t rb = (((p.c0 & 0xFF00FFu) * mq + (f.c0 & 0xFF00FFu) * nq + 0x800080u) >> 8) & 0xFF00FFu;
    const uint32_t gr = ((((p.c0 >> 8) & 0xFFu) * mq + ((f.c0 >> 8) & 0xFFu) * nq + 128u) >> 8) << 8;
    ViewPx<uint8_t> o;
    o.c0 = rb | gr;
    return o;
}
__device__ __forceinline__ uint32_t rise_blend_word(uint32_t pb, uint32_t fb, uint32_t mq, float w) {
    const float p = __uint_as_float(pb), f = __uint_as_float(fb);
    const uint32_t v = __float_as_uint(__fadd_rn(f, __fmul_rn(w, __fsub_rn(p, f))));
    return mq == 256u ? pb : (mq == 0u ? fb : v);
}
__device__ __forceinline__ ViewPx<uint32_t> rise_blend(const ViewPx<uint32_t> p, const ViewPx<uint32_t> f, uint32_t mq) {
    const float w = __fmul_rn((float)mq, 0x1p-8f);
    ViewPx<uint32_t> o;
    o.c0 = rise_blend_word(p.c0, f.c0, mq, w);
    o.c1 = rise_blend_word(p.c1, f.c1, mq, w);
    o.c2 = rise_blend_word(p.c2, f.c2, mq, w);
    return o;
}

// ---- the mask kernel.  Work items and grid as in occlude_kernel: item = (row y, group g) of a frame, block b of the grid-stride
// loop is part b % parts of frame b / parts.  An item loads its source pixels once; for every chunk of masks the block draws the
// grid rows and shifts into LDS, then every item blends and stores its group once a mask.  Every loop bound around a barrier is
// uniform in the block: an item without pixels skips the work, never the barrier.
template <class U>
__global__ __launch_bounds__(256) void rise_mask_kernel(const U* __restrict__ in, U* __restrict__ out, int n, int H, int W, RiseArg ra,
                                                        const uint32_t fill0, const uint32_t fill1, const uint32_t fill2, int m0, int m1,
                                                        int parts, FastDiv div_g, long long blocks, const U* lo, const U* hi) {
    using Px = ViewPx<U>;
    __shared__ uint32_t rows[RISE_MASK_CHUNK][16];
    __shared__ int2 shift[RISE_MASK_CHUNK];
    const int G = (int)div_g.d;
    const uint32_t items = (uint32_t)H * (uint32_t)G;
    const size_t row_units = (size_t)W * 3;
    const size_t mask_units = (size_t)n * H * row_units;
    const uint32_t fw[3] = {fill0, fill1, fill2};
    Px fill;
    vpx_fill(fill, fw);
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long i = blk / parts;                             // uniform: the frame
        const uint32_t F = ra.first + (uint32_t)i;
        const uint32_t t = (uint32_t)(blk - i * parts) * 256u + threadIdx.x;
        bool active = t < items;
        int y = 0, x0 = 0, k = 0;
        U* orow = out;
        Px p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vpx_zero(p[j]);
        if (active) {
            y = (int)fastdiv(t, div_g);
            const int g = (int)(t - (uint32_t)y * (uint32_t)G);
            const size_t row_off = ((size_t)i * H + y) * row_units;
            orow = out + row_off;
            const int al = (int)(((uintptr_t)orow / sizeof(U)) & 3);
            const PxGroup grp = px_group(al, g, W);
            k = grp.k;
            x0 = (int)grp.p0;
            active = k != 0;
            if (active) {
                const U* s = in + row_off + 3 * (size_t)x0;
                if (k == 4) {
                    vgroup_load(s, lo, hi, p);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < k) p[j] = vpx_load(s + 3 * j);
                }
            }
        }
        for (int mc = m0; mc < m1; mc += RISE_MASK_CHUNK) {
            const int cnt = min(RISE_MASK_CHUNK, m1 - mc);
            __syncthreads();                                         // the items are done with the chunk before
            rise_stage(ra, F, mc, cnt, rows, shift, (int)threadIdx.x, 256);
            __syncthreads();
            if (!active) continue;
            for (int ms = 0; ms < cnt; ++ms) {
                const int2 sh = shift[ms];
                const RiseAxis ay = rise_axis(y + sh.x, ra.ch, ra.ch2, ra.div_ch2, ra.g);
                const uint32_t r0 = rows[ms][ay.i0], r1 = rows[ms][ay.i1];
                Px q[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const RiseAxis ax = rise_axis(x0 + j + sh.y, ra.cw, ra.cw2, ra.div_cw2, ra.g);
                    q[j] = rise_blend(p[j], fill, rise_mq(ra, r0, r1, ay, ax));
                }
                U* o = orow + (size_t)(mc + ms - m0) * mask_units + 3 * (size_t)x0;
                if (k == 4 && (((uintptr_t)o / sizeof(U)) & 3) == 0) {
                    vgroup_store(o, q);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < k) vpx_store(o + 3 * j, q[j]);
                }
            }
        }
    }
}

// ---- the accumulate head: a block a frame.  prob is [N + 1][n] planes, map [n][mh * mw], rec [n] records of eight dwords.
struct RiseAccParams {
    const float* prob;
    const int* classes;
    float* map;
    int32_t* rec;
    RiseArg ra;
    int n, N, H, W, mh, mw;
    int num_classes;           // 0: not known (fav_op_rise_accumulate may say so) - only a negative class is then out of range
    float inv_n;               // (float)(1.0 / N)
};

// the sample pixel of cell c of m along an axis of `size` pixels: the middle of the pixels p with p * m / size == c
__device__ __forceinline__ int rise_sample(int c, int size, int m) {
    const long long lo = ((long long)c * size + m - 1) / m, hi = ((long long)(c + 1) * size + m - 1) / m - 1;
    return (int)((lo + hi) / 2);
}

__global__ __launch_bounds__(RISE_ACC_THREADS) void rise_accumulate_kernel(const RiseAccParams p) {
    __shared__ uint32_t rows[RISE_ACC_CHUNK][16];
    __shared__ int2 shift[RISE_ACC_CHUNK];
    __shared__ float pr[RISE_ACC_CHUNK];
    __shared__ float m_s[CV_MAX_CELLS];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int cells = p.mh * p.mw;
    const RiseArg& ra = p.ra;
    const uint32_t F = ra.first + (uint32_t)i;
    int yc[4], xc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = tid + RISE_ACC_THREADS * k;
        yc[k] = xc[k] = 0;
        if (c < cells) {
            const int cy = c / p.mw;
            yc[k] = rise_sample(cy, p.H, p.mh);
            xc[k] = rise_sample(c - cy * p.mw, p.W, p.mw);
        }
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t cov[4] = {0u, 0u, 0u, 0u};
    float psum = 0.f;                                                // every thread carries the same chain
    for (int mc = 0; mc < p.N; mc += RISE_ACC_CHUNK) {
        const int cnt = min(RISE_ACC_CHUNK, p.N - mc);
        __syncthreads();
        rise_stage(ra, F, mc, cnt, rows, shift, tid, RISE_ACC_THREADS);
        if (tid < cnt) pr[tid] = p.prob[(size_t)(1 + mc + tid) * p.n + i];
        __syncthreads();
        for (int ms = 0; ms < cnt; ++ms) {
            const float pm = pr[ms];
            const int2 sh = shift[ms];
            psum = __fadd_rn(psum, pm);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (tid + RISE_ACC_THREADS * k >= cells) continue;
                const RiseAxis ay = rise_axis(yc[k] + sh.x, ra.ch, ra.ch2, ra.div_ch2, ra.g);
                const RiseAxis ax = rise_axis(xc[k] + sh.y, ra.cw, ra.cw2, ra.div_cw2, ra.g);
                const uint32_t wq = rise_mq(ra, rows[ms][ay.i0], rows[ms][ay.i1], ay, ax);
                acc[k] = __fadd_rn(acc[k], __fmul_rn(pm, __fmul_rn((float)wq, 0x1p-8f)));
                cov[k] += wq;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = tid + RISE_ACC_THREADS * k;
        if (c >= cells) continue;
        const float v = cov[k] > 0u ? __fdiv_rn(acc[k], __fmul_rn((float)cov[k], 0x1p-8f)) : 0.f;
        m_s[c] = v;
        p.map[(size_t)i * cells + c] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    // the record, by one lane: serial scans in index order (steps 5 and 6 of fav_rollout_record)
    int32_t* const rec = p.rec + 8 * (size_t)i;
    const int cls = p.classes[i];
    if (cls < 0 || (p.num_classes > 0 && cls >= p.num_classes)) {
        map_record_no_class(rec, 0, -1);
        return;
    }
    float peak = -INFINITY, flo = INFINITY;
    int peak_cell = -1, n_above = 0, box = -1;
    for (int c = 0; c < cells; ++c) {
        const float v = m_s[c];
        if (v > peak) { peak = v; peak_cell = c; }
        if (v < flo) flo = v;
    }
    if (peak > flo) n_above = map_box_scan(m_s, cells, p.mw, __fadd_rn(flo, __fmul_rn(0.5f, __fsub_rn(peak, flo))), &box);
    map_record_store(rec, cls, __float_as_int(p.prob[i]), __float_as_int(peak), peak_cell, __float_as_int(flo),
                     __float_as_int(__fmul_rn(psum, p.inv_n)), n_above, box);
}

}  // namespace fav
