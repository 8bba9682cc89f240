// fav_curve.hpp - deletion / insertion curves behind fav_op_rank_cells, fav_op_occlude, fav_op_head_class_prob, fav_op_curve and
// fav_set_curve / fav_classify_curve (include/fav.h).  A saliency map of at most 1024 cells is
// ranked, the frames are occluded cell by cell in that order, every step is classified again and the probability of one class is
// integrated over the steps.  Four kernels, one launch each:
//   rank_cells_kernel       a block a frame: the map in LDS, a thread counts the cells in front of its own
//   occlude_kernel          pure data movement on [H][W][3] frames of either layout: four neighbouring pixels a work item, the
//                           source group loaded once and stored once a step - three dwords (u8) or three 16-byte words (f32)
//   head_class_prob_kernel  the heads' shared core (fav_kernels.hpp), then pbar of a named class
//   curve_kernel            a thread a frame: the fixed-order chains over the steps, a record of eight dwords
// Included by fav.hip after fav_views.hpp (ViewPx, vgroup_load / vgroup_store), fav_corrupt_c.hpp (px_group), fav_route.hpp
// (fmt) and fav_mapbox.hpp (map_record_store), and in front of fav_rise.hpp, whose head shares the host steps in fav.hip
// (perturb_clear .. classify_perturb_head, row_groups, fill_words, stream_out_error) and map_record_no_class below.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int CV_MAX_CELLS = 1024;         // cells of a map: the ranks of a frame are 4 KB of LDS
constexpr int CV_MAX_SIDE = 256;
constexpr int CV_MAX_STEPS = 256;
constexpr int CV_CURVE_THREADS = 64;

// ---- host: the one place the ranges live
inline std::string curve_steps_error(int S) {
    if (S < 1 || S > CV_MAX_STEPS) return fmt("steps=%d outside [1, %d]", S, CV_MAX_STEPS);
    return std::string();
}
inline std::string curve_map_error(int mh, int mw) {
    if (mh < 1 || mw < 1 || mh > CV_MAX_SIDE || mw > CV_MAX_SIDE || mh * mw > CV_MAX_CELLS)
        return fmt("map %dx%d: needs 1 <= mh, mw <= %d and mh * mw <= %d cells", mh, mw, CV_MAX_SIDE, CV_MAX_CELLS);
    return std::string();
}
inline std::string curve_mode_error(int mode) {
    if (mode != FAV_CURVE_DELETION && mode != FAV_CURVE_INSERTION) return fmt("mode=%d is not a fav_curve_mode value", mode);
    return std::string();
}
// a fill against a layout: a byte a channel under u8; any word is the bits of an fp32
inline std::string curve_fill_error(const uint32_t* fill, int layout) {
    if (layout == FAV_LAYOUT_NHWC_U8)
        for (int c = 0; c < 3; ++c)
            if (fill[c] > 255u) return fmt("fill[%d]=%u is above 255, the largest uint8", c, fill[c]);
    return std::string();
}
inline std::string curve_frame_error(int H, int W, int layout) {
    if (H < 1 || W < 1) return fmt("frame size %dx%d: H and W must be at least 1", H, W);
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return "unknown layout";
    // the occlusion kernel holds a frame's work items in 32 bits, as the view kernels do
    if ((long long)H * W > 0x7FFFFFFFll / 12) return "H * W above (2^31 - 1) / 12 pixels";
    return std::string();
}
// fav_check_curve: the descriptor for H x W frames of `layout`
inline std::string curve_desc_error(const fav_curve* d, int H, int W, int layout) {
    if (!d) return "desc is NULL";
    if (d->struct_size != sizeof(fav_curve)) return "struct_size is not sizeof(fav_curve)";
    std::string why = curve_steps_error(d->steps);
    if (why.empty()) why = curve_frame_error(H, W, layout);
    if (why.empty() && layout == FAV_LAYOUT_NHWC_U8) why = curve_fill_error(d->fill_u8, layout);
    return why;
}

// ---- rank: rank[c] = the number of cells in front of c.  a stands in front of c when c is NaN and a is not, when both are
//      numbers and M[a] > M[c], and when neither is greater (equal, +0 against -0, both NaN) and a < c.
__global__ __launch_bounds__(256) void rank_cells_kernel(const float* __restrict__ map, int cells, int* __restrict__ rank) {
    __shared__ float m[CV_MAX_CELLS];
    const float* src = map + (size_t)blockIdx.x * cells;
    for (int c = threadIdx.x; c < cells; c += 256) m[c] = src[c];
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {
        const float v = m[c];
        const bool vn = v != v;
        int r = 0;
        for (int a = 0; a < cells; ++a) {       // every lane reads the same word: a broadcast
            const float w = m[a];
            const bool wn = w != w;
            const bool front = vn ? (!wn || a < c) : (w > v || (w == v && a < c));
            r += front ? 1 : 0;
        }
        rank[(size_t)blockIdx.x * cells + c] = r;
    }
}

// ---- occlusion.  Work items as in views_straight_kernel: item = (row y, group g) of a frame, the groups of px_group along the
// row laid out by the alignment of the row in the launch's FIRST step; block b of the grid-stride loop is part b % parts of frame
// b / parts.  A block stages its frame's ranks in LDS when the frame changes, an item loads its source pixels once and stores
// them, or the fill, once a step.  A later step whose frames lie at another alignment (n * H * W * 3 no multiple of 4) stores
// its groups pixel by pixel.
struct OccludeArg {
    uint32_t fill[3];
    int mode, S, s0, s1, mh, mw, cells;
    int wide;                  // H or W above 2^23: y * mh does not fit the 32-bit division
    FastDiv div_h, div_w;
};

__device__ __forceinline__ void vpx_fill(ViewPx<uint8_t>& f, const uint32_t (&w)[3]) { f.c0 = w[0] | (w[1] << 8) | (w[2] << 16); }
__device__ __forceinline__ void vpx_fill(ViewPx<uint32_t>& f, const uint32_t (&w)[3]) { f.c0 = w[0]; f.c1 = w[1]; f.c2 = w[2]; }

// v * m / d in integer division
__device__ __forceinline__ int cell_index(int v, int m, const FastDiv& d, int wide) {
    if (wide) return (int)((unsigned long long)v * (unsigned long long)m / d.d);
    return (int)fastdiv((uint32_t)v * (uint32_t)m, d);
}

template <class U>
__global__ __launch_bounds__(256) void occlude_kernel(const U* __restrict__ in, U* __restrict__ out, const int* __restrict__ rank,
                                                      int n, int H, int W, OccludeArg oa, int parts, FastDiv div_g, long long blocks,
                                                      const U* lo, const U* hi) {
    using Px = ViewPx<U>;
    __shared__ int rk[CV_MAX_CELLS];
    const int G = (int)div_g.d;
    const uint32_t items = (uint32_t)H * (uint32_t)G;
    const size_t row_units = (size_t)W * 3;
    const size_t step_units = (size_t)n * H * row_units;
    Px fill;
    vpx_fill(fill, oa.fill);
    long long staged = -1;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long i = blk / parts;                             // uniform: the frame
        if (i != staged) {
            __syncthreads();                                         // the items of the frame before are done with rk
            for (int c = threadIdx.x; c < oa.cells; c += 256) rk[c] = rank[(size_t)i * oa.cells + c];
            __syncthreads();
            staged = i;
        }
        const uint32_t t = (uint32_t)(blk - i * parts) * 256u + threadIdx.x;
        if (t >= items) continue;
        const int y = (int)fastdiv(t, div_g), g = (int)(t - (uint32_t)y * (uint32_t)G);
        const size_t row_off = ((size_t)i * H + y) * row_units;
        U* orow = out + row_off;
        const int al = (int)(((uintptr_t)orow / sizeof(U)) & 3);
        const PxGroup grp = px_group(al, g, W);
        if (!grp.k) continue;
        const int x0 = (int)grp.p0;
        const U* s = in + row_off + 3 * (size_t)x0;
        Px p[4];
        int r[4];
        const int cy = cell_index(y, oa.mh, oa.div_h, oa.wide) * oa.mw;
        if (grp.k == 4) {
            vgroup_load(s, lo, hi, p);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vpx_zero(p[j]);
                if (j < grp.k) p[j] = vpx_load(s + 3 * j);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = j < grp.k ? rk[cy + cell_index(x0 + j, oa.mw, oa.div_w, oa.wide)] : 0;
        for (int st = oa.s0; st < oa.s1; ++st) {
            const int k = st * oa.cells / oa.S;                      // uniform
            U* o = orow + (size_t)(st - oa.s0) * step_units + 3 * (size_t)x0;
            Px q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = ((r[j] < k) == (oa.mode == FAV_CURVE_DELETION)) ? fill : p[j];
            if (grp.k == 4 && (((uintptr_t)o / sizeof(U)) & 3) == 0) {
                vgroup_store(o, q);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < grp.k) vpx_store(o + 3 * j, q[j]);
            }
        }
    }
}

// ---- the class-probability head: pbar, the label and the non-finite flag exactly as head_kernel computes them (the head
// core), then prob = pbar[classes[img]] (classes NULL: the frame's own label, so prob is head_unc_kernel's mean_prob).  A class
// outside [0, C) and a non-finite frame give NaN; labels may be NULL.
template <int NV>
__global__ __launch_bounds__(256) void head_class_prob_kernel(const float* __restrict__ logits, int T, int n, int C, int ld,
                                                              float inv_temp, const int* __restrict__ classes,
                                                              float* __restrict__ prob, int* __restrict__ labels) {
    __shared__ __attribute__((aligned(16))) float part[4][NV * 256];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ float red_h[4];
    const int img = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float p[NV][4] = {};
    for (int t = wave; t < T; t += 4) {
        float z[NV][4];
        const float mx = head_load_row(logits + ((long long)t * n + img) * ld, C, inv_temp, lane, z);
        head_accumulate<false>(z, mx, p);
    }
    float pb[4], own[4], best, bv;
    int besti, bi;
    head_combine<NV>(part, p, tid, C, 1.0f / (float)T, pb, red_h);
#pragma unroll
    for (int j = 0; j < 4; ++j) own[j] = pb[j];
    head_mask_classes(pb, tid, C);
    head_thread_argmax(pb, tid, best, besti);
    wave_argmax(best, besti);
    if (lane == 0) { red_v[wave] = best; red_i[wave] = besti; }
    __syncthreads();
    argmax_of_waves(red_v, red_i, bv, bi);
    const bool bad = head_nonfinite(bv);
    const int label = bad ? 0 : bi;
    const int cls = classes ? classes[img] : label;
    const bool in_range = cls >= 0 && cls < C;
    if (tid == 0 && labels) labels[img] = label;
    if (tid == (in_range ? cls >> 2 : 0)) {      // the thread that holds pbar of the class
        float v = own[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if ((cls & 3) == j) v = own[j];
        prob[img] = in_range && !bad ? v : __int_as_float(0x7fc00000);
    }
}

// a class outside the range has no curve and no map (curve_kernel, rise_accumulate_kernel): its record is class -1 with NaN in
// the four fp32 fields and cell -1, then the head's own two last dwords
__device__ __forceinline__ void map_record_no_class(int32_t* rec, int d6, int d7) {
    const int nan = 0x7fc00000;
    map_record_store(rec, -1, nan, nan, -1, nan, nan, d6, d7);
}

// ---- the curve: a thread a frame, every chain in step order.  prob / labels are [S + 1][n] planes, curve is [n][S + 1].
struct CurveParams {
    const float* prob;
    const int* labels;
    const int* classes;
    float* curve;
    int32_t* rec;
    int n, S, cells, mode;
    int num_classes;           // 0: not known (fav_op_curve) - only a negative class is then out of range
    float half_step;           // (float)(0.5 / S)
};

__global__ __launch_bounds__(CV_CURVE_THREADS) void curve_kernel(const CurveParams cp) {
    const int i = blockIdx.x * CV_CURVE_THREADS + threadIdx.x;
    if (i >= cp.n) return;
    const int cls = cp.classes[i];
    const int S = cp.S;
    float acc = 0.f, pmin = INFINITY, prev = 0.f, first = 0.f;
    int flip = -1;
    for (int s = 0; s <= S; ++s) {
        const float p = cp.prob[(size_t)s * cp.n + i];
        cp.curve[(size_t)i * (S + 1) + s] = p;
        if (s == 0) first = p; else acc = acc + (prev + p);
        if (p < pmin) pmin = p;
        const bool same = cp.labels[(size_t)s * cp.n + i] == cls;
        if (flip < 0 && same == (cp.mode == FAV_CURVE_INSERTION)) flip = s;
        prev = p;
    }
    const float auc = acc * cp.half_step;
    int32_t* const rec = cp.rec + (size_t)i * 8;
    if (cls < 0 || (cp.num_classes > 0 && cls >= cp.num_classes)) {
        map_record_no_class(rec, -1, 0);
        return;
    }
    map_record_store(rec, cls, __float_as_int(auc), __float_as_int(first), flip, __float_as_int(prev), __float_as_int(pmin),
                     flip < 0 ? -1 : flip * cp.cells / S, 0);
}

}  // namespace fav
