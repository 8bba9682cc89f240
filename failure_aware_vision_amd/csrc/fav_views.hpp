// fav_views.hpp - test-time-augmentation views behind fav_op_views and fav_set_views (include/fav.h; DESIGN.md section 2,
// item 5e).  A view is pure data movement on [H][W][3] frames of either layout: out[y][x] = in[u][v] with
//   (u, v) = (y - dy, x - dx) -> border rule against (H, W) -> flip_y / flip_x -> swap when `transpose`,
// every element copied bit for bit (an fp32 NaN keeps its payload: the kernels move uint32 words).  out is [n_views][n][H][W][3].
// Included by fav.hip after fav_corrupt_c.hpp (px_group, reflect101) and fav_route.hpp (fmt).
//
//   straight views   : views_straight_kernel, four neighbouring output pixels a thread - three dwords (u8) or three 16-byte
//                      words (f32) out; an x flip reverses the pixels of the group, not its bytes
//   transposed views : views_transpose_kernel, a 32 x 32 pixel tile through LDS, loads and stores both along rows
// Both kernels are written once over the element type U (uint8_t / uint32_t): a pixel is 3 units, a store word V (uint32_t /
// uint4) is 4 units, so a group of four pixels is three store words in either layout.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int VW_MAX_VIEWS = 64;
constexpr int VW_TILE = 32;                              // pixel edge of the transposed kernel's tile
constexpr int VW_SLOTS = VW_TILE * 3 / 4 + 1;            // 25: store words that a tile row of 96 units can touch
// the tile's row stride in units: 97 dwords (f32: a column read walks the banks one by one), 100 bytes (u8: 25 dwords, odd)
template <class U> struct ViewUnit;
template <> struct ViewUnit<uint8_t> { using V = uint32_t; static constexpr int LD = VW_TILE * 3 + 4; };
template <> struct ViewUnit<uint32_t> { using V = uint4; static constexpr int LD = VW_TILE * 3 + 1; };

// what a launch gets: every view of the call and the `count` of them this launch makes (their positions in `v`)
struct ViewsArg {
    fav_view v[VW_MAX_VIEWS];
    uint8_t idx[VW_MAX_VIEWS];
    int count;
};

// ---- host: the one place the ranges live (fav_check_views)
inline std::string views_error(const fav_view* views, int n_views, int H, int W) {
    if (!views) return "views is NULL";
    if (n_views < 1 || n_views > VW_MAX_VIEWS) return fmt("n_views=%d outside [1, FAV_MAX_VIEWS=%d]", n_views, VW_MAX_VIEWS);
    if (H < 1 || W < 1) return fmt("frame size %dx%d: H and W must be at least 1", H, W);
    for (int a = 0; a < n_views; ++a) {
        const fav_view& v = views[a];
        if (v.flip_x != 0 && v.flip_x != 1) return fmt("view %d: flip_x=%d is not 0 or 1", a, v.flip_x);
        if (v.flip_y != 0 && v.flip_y != 1) return fmt("view %d: flip_y=%d is not 0 or 1", a, v.flip_y);
        if (v.transpose != 0 && v.transpose != 1) return fmt("view %d: transpose=%d is not 0 or 1", a, v.transpose);
        if (v.dy < -65535 || v.dy > 65535) return fmt("view %d: dy=%d outside [-65535, 65535]", a, v.dy);
        if (v.dx < -65535 || v.dx > 65535) return fmt("view %d: dx=%d outside [-65535, 65535]", a, v.dx);
        if (v.border < FAV_BORDER_REFLECT101 || v.border > FAV_BORDER_ZERO) return fmt("view %d: border=%d is not a fav_border value", a, v.border);
        if (v.transpose && H != W) return fmt("view %d: transpose needs H == W, the frames are %dx%d", a, H, W);
    }
    return std::string();
}

// ---- device: source index of output index i - d along a dimension of n, or -1 where FAV_BORDER_ZERO leaves the frame
__device__ __forceinline__ int view_src(int i, int n, int border, int flip) {
    int s;
    if (border == FAV_BORDER_REFLECT101) s = reflect101(i, n);
    else if (border == FAV_BORDER_REPLICATE) s = min(max(i, 0), n - 1);
    else if (i < 0 || i >= n) return -1;
    else s = i;
    return flip ? n - 1 - s : s;
}

// a pixel in registers: 24 bits of one word (u8) or three words (f32)
template <class U> struct ViewPx;
template <> struct ViewPx<uint8_t> { uint32_t c0; };
template <> struct ViewPx<uint32_t> { uint32_t c0, c1, c2; };

__device__ __forceinline__ ViewPx<uint8_t> vpx_load(const uint8_t* p) {
    ViewPx<uint8_t> r;
    r.c0 = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return r;
}
__device__ __forceinline__ ViewPx<uint32_t> vpx_load(const uint32_t* p) {
    ViewPx<uint32_t> r;
    r.c0 = p[0]; r.c1 = p[1]; r.c2 = p[2];
    return r;
}
__device__ __forceinline__ void vpx_store(uint8_t* p, const ViewPx<uint8_t> v) {
    p[0] = (uint8_t)v.c0; p[1] = (uint8_t)(v.c0 >> 8); p[2] = (uint8_t)(v.c0 >> 16);
}
__device__ __forceinline__ void vpx_store(uint32_t* p, const ViewPx<uint32_t> v) { p[0] = v.c0; p[1] = v.c1; p[2] = v.c2; }
__device__ __forceinline__ void vpx_zero(ViewPx<uint8_t>& v) { v.c0 = 0; }
__device__ __forceinline__ void vpx_zero(ViewPx<uint32_t>& v) { v.c0 = v.c1 = v.c2 = 0; }

// Four neighbouring source pixels from s.  u8: the 12 bytes lie in three or four aligned dwords, which are loaded whole and
// shifted into place - only when every one of them lies inside the call's frames [lo, hi) (both dword aligned inwards);
// otherwise, as for f32 rows that are not 16-byte aligned, unit by unit.
__device__ __forceinline__ void vgroup_load(const uint8_t* s, const uint8_t* lo, const uint8_t* hi, ViewPx<uint8_t> (&p)[4]) {
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
    const uint8_t* b = s - sh;
    if (b >= lo && b + (sh ? 16 : 12) <= hi) {
        const uint32_t* q = (const uint32_t*)b;
        uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        if (sh) {
            const uint32_t w3 = q[3], r = 8 * sh, l = 32 - r;
            w0 = (w0 >> r) | (w1 << l);
            w1 = (w1 >> r) | (w2 << l);
            w2 = (w2 >> r) | (w3 << l);
        }
        p[0].c0 = w0 & 0xFFFFFFu;
        p[1].c0 = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
        p[2].c0 = (w1 >> 16) | ((w2 & 0xFFu) << 16);
        p[3].c0 = w2 >> 8;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = vpx_load(s + 3 * j);
}
__device__ __forceinline__ void vgroup_load(const uint32_t* s, const uint32_t*, const uint32_t*, ViewPx<uint32_t> (&p)[4]) {
    if (((uintptr_t)s & 15) == 0) {
        const uint4* q = (const uint4*)s;
        const uint4 a = q[0], b = q[1], c = q[2];
        p[0].c0 = a.x; p[0].c1 = a.y; p[0].c2 = a.z;
        p[1].c0 = a.w; p[1].c1 = b.x; p[1].c2 = b.y;
        p[2].c0 = b.z; p[2].c1 = b.w; p[2].c2 = c.x;
        p[3].c0 = c.y; p[3].c1 = c.z; p[3].c2 = c.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = vpx_load(s + 3 * j);
}
// four pixels as three store words; o is aligned for V
__device__ __forceinline__ void vgroup_store(uint8_t* o, const ViewPx<uint8_t> (&p)[4]) {
    uint32_t* q = (uint32_t*)o;
    q[0] = p[0].c0 | (p[1].c0 << 24);
    q[1] = (p[1].c0 >> 8) | (p[2].c0 << 16);
    q[2] = (p[2].c0 >> 16) | (p[3].c0 << 8);
}
__device__ __forceinline__ void vgroup_store(uint32_t* o, const ViewPx<uint32_t> (&p)[4]) {
    uint4* q = (uint4*)o;
    q[0] = make_uint4(p[0].c0, p[0].c1, p[0].c2, p[1].c0);
    q[1] = make_uint4(p[1].c1, p[1].c2, p[2].c0, p[2].c1);
    q[2] = make_uint4(p[2].c2, p[3].c0, p[3].c1, p[3].c2);
}

// ---- straight views.  One work item is four neighbouring pixels of one output row: item = (row y, group g), with the groups
// of px_group along the row, G = 1 + ceil(W / 4) of them.  Group 0 is the pixels in front of the row's first pixel whose
// output address is aligned for V (none to three of them); group g >= 1 is the four pixels from there on, fewer at the row's
// end.  A full group whose four sources lie inside the source row is one contiguous run of that row, reversed by an x flip;
// a group that touches the border, the head and the tail go pixel by pixel.
// The grid: an output frame (frame i under straight view sa) has H * G items and takes `parts` blocks of 256 items.  Block b
// of the grid-stride loop is part b % parts of output frame b / parts, and output frames are numbered frame by frame with a
// frame's views side by side, so the frame comes from HBM for the first of its views and from the cache for the others.
template <class U>
__global__ __launch_bounds__(256) void views_straight_kernel(const U* __restrict__ in, U* __restrict__ out, int n, int H, int W,
                                                             ViewsArg va, int parts, FastDiv div_g, long long blocks,
                                                             const U* lo, const U* hi) {
    using Px = ViewPx<U>;
    const int G = (int)div_g.d;
    const uint32_t items = (uint32_t)H * (uint32_t)G;
    const size_t row_units = (size_t)W * 3;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long of = blk / parts;                            // uniform: frame of / count, straight view of % count
        const uint32_t t = (uint32_t)(blk - of * parts) * 256u + threadIdx.x;
        if (t >= items) continue;
        const int i = (int)(of / va.count), sa = (int)(of - (long long)i * va.count);
        const int a = va.idx[sa];
        const fav_view vw = va.v[a];
        const int y = (int)fastdiv(t, div_g), g = (int)(t - (uint32_t)y * (uint32_t)G);
        U* orow = out + (((size_t)a * n + i) * H + y) * row_units;
        const int al = (int)(((uintptr_t)orow / sizeof(U)) & 3);
        const PxGroup grp = px_group(al, g, W);
        if (!grp.k) continue;
        const int x0 = (int)grp.p0;
        U* o = orow + 3 * (size_t)x0;
        const int u = view_src(y - vw.dy, H, vw.border, vw.flip_y);
        Px p[4];
        if (u < 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) vpx_zero(p[j]);
        } else {
            const U* srow = in + ((size_t)i * H + u) * row_units;
            const int v0 = x0 - vw.dx;
            if (grp.k == 4 && v0 >= 0 && v0 + 3 < W) {
                vgroup_load(srow + 3 * (size_t)(vw.flip_x ? W - 4 - v0 : v0), lo, hi, p);
                if (vw.flip_x) {
                    const Px t0 = p[0], t1 = p[1];
                    p[0] = p[3]; p[1] = p[2]; p[2] = t1; p[3] = t0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    vpx_zero(p[j]);
                    if (j < grp.k) {
                        const int v = view_src(v0 + j, W, vw.border, vw.flip_x);
                        if (v >= 0) p[j] = vpx_load(srow + 3 * (size_t)v);
                    }
                }
            }
        }
        if (grp.k == 4) {
            vgroup_store(o, p);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < grp.k) vpx_store(o + 3 * j, p[j]);
        }
    }
}

// ---- transposed views (H == W == S): out[y][x] = in[fx(x)][fy(y)].  Per 32 x 32 tile of the output: thread (j, t) loads the
// source pixel of output (y0 + t, x0 + j) - consecutive lanes walk along a source row - into tile[j][t]; then output row
// ty is read out of the tile's column ty (row stride LD: 97 dwords or 25 dwords, so a column read falls on different banks)
// and stored in words of four units: slot k of a row covers units 4k - mis .. 4k - mis + 3 of the tile row, mis the
// misalignment of the tile row's first unit; a slot that is not wholly inside the tile row stores its units one by one
// (the neighbouring tile writes the others).  LDS: 3200 bytes (u8), 12 416 bytes (f32).
template <class U>
__global__ __launch_bounds__(256) void views_transpose_kernel(const U* __restrict__ in, U* __restrict__ out, int n, int S,
                                                              ViewsArg va, int tiles_1d, long long tiles) {
    using Px = ViewPx<U>;
    using V = typename ViewUnit<U>::V;
    constexpr int LD = ViewUnit<U>::LD;
    __shared__ __align__(16) U tile[VW_TILE * LD];
    const size_t row_units = (size_t)S * 3;
    const int per_frame = tiles_1d * tiles_1d;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long long of = tl / per_frame;
        const int rest = (int)(tl - of * per_frame);
        const int ty_ = rest / tiles_1d, y0 = ty_ * VW_TILE, x0 = (rest - ty_ * tiles_1d) * VW_TILE;
        const int i = (int)(of / va.count), sa = (int)(of - (long long)i * va.count);
        const int a = va.idx[sa];
        const fav_view vw = va.v[a];
        const U* fin = in + (size_t)i * S * row_units;
        for (int e = threadIdx.x; e < VW_TILE * VW_TILE; e += 256) {
            const int j = e / VW_TILE, t = e - j * VW_TILE;
            const int x = x0 + j, y = y0 + t;
            if (x < S && y < S) {
                const int r = view_src(x - vw.dx, S, vw.border, vw.flip_x);   // the source row comes from x,
                const int c = view_src(y - vw.dy, S, vw.border, vw.flip_y);   // the source column from y
                Px p;
                vpx_zero(p);
                if (r >= 0 && c >= 0) p = vpx_load(fin + (size_t)r * row_units + 3 * (size_t)c);
                vpx_store(tile + j * LD + 3 * t, p);
            }
        }
        __syncthreads();
        const int tw3 = min(VW_TILE, S - x0) * 3;                    // units of a tile row
        for (int e = threadIdx.x; e < VW_TILE * VW_SLOTS; e += 256) {
            const int ty = e / VW_SLOTS, k = e - ty * VW_SLOTS;
            const int y = y0 + ty;
            if (y >= S) continue;
            U* seg = out + (((size_t)a * n + i) * S + y) * row_units + 3 * (size_t)x0;
            const int mis = (int)(((uintptr_t)seg / sizeof(U)) & 3);
            const int e0 = 4 * k - mis;
            if (e0 >= tw3) continue;
            U w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int eu = e0 + q;
                const int px = eu / 3, ch = eu - 3 * px;
                w[q] = (eu >= 0 && eu < tw3) ? tile[px * LD + 3 * ty + ch] : (U)0;
            }
            if (e0 >= 0 && e0 + 4 <= tw3) {
                if constexpr (sizeof(U) == 1)
                    *(V*)(seg + e0) = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
                else
                    *(V*)(seg + e0) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e0 + q >= 0 && e0 + q < tw3) seg[e0 + q] = w[q];
            }
        }
        __syncthreads();
    }
}

}  // namespace fav
