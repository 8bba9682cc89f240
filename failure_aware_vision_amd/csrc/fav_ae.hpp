// fav_ae.hpp - the autoencoder anomaly sensor behind fav_ae_* and fav_op_ae_decode_compare (include/fav.h; DESIGN.md section 2,
// item 5p).  A convolutional autoencoder trained on normal frames only; the frame's score is the mean squared error of its
// reconstruction, the error map says where.  The encoder and every decoder layer but the last are launches the library has
// (stem im2col, the convolution launcher); what is new is the last layer: a 2x2 / stride-2 transposed convolution 64 -> 3,
// the sigmoid, the byte, the comparison with the frame and the reduction to cells and a record.  The contract (fav.h, beside
// fav_ae_record) fixes every operation up to the integer error, and integer sums have no order, so the result is the bits of
// a numpy restatement (tests/ae_ref.py).
// Included by fav.hip after fav_kernels.hpp (fav_expf, fav_sanitize_px, the MFMA vector types), fav_route.hpp (fmt) and
// fav_mapbox.hpp (the box scan and the record store).
//
//   ae_decode_kernel<LAYOUT>  : a block a cell of a frame.  The cell's (cell / 2)^2 level-1 pixels are 1, 4 or 16 tiles of 16
//                               hidden rows, a wave a tile at a time; a lane finds its row from the pixel (the row order of
//                               the GEMM decode steps is the Morton code of the pixel's low m bits under the coarse pixel) and
//                               loads its A fragment straight from global memory, 16 bytes a K half; the 12 weight rows are
//                               the B fragment, loaded once.  Two MFMAs a tile.  A lane then holds one output column
//                               (a, b, channel) of four rows: bias, sigmoid, byte, the frame's byte, the squared difference.
//                               Pixels beyond the frame are computed and dropped.  The cell's sum goes through a wave
//                               reduction and LDS to one store: no atomics, no block waits for another.
//   ae_record_kernel          : a block a frame, a thread a cell: the cell's mean from its integer sum (the first kernel left
//                               the sums where the means go, so the head needs no workspace), then one lane's serial scans
//                               in index order as in cam_kernel: the 64-bit frame sum, the peak and the floor, map_box_scan.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int AE_MAX_LEVELS = 3, AE_MAX_SIDE = 4096, AE_MAX_CELLS = 1024, AE_MAX_GRID_SIDE = 256;
constexpr int AE_REC_THREADS = 1024;
constexpr size_t AE_MAX_WORKSPACE = (size_t)1 << 30;
constexpr uint32_t AE_BLOB_MAGIC = 0x41564146u;              // "FAVA" little endian
constexpr size_t AE_BLOB_HEADER = 64, AE_BLOB_ALIGN = 64;

inline int ae_width(int level) { return 64 << (level - 1); }    // C_l, l = 1 .. 3

// ---- host: the one place the geometry lives
struct AeGeom {
    int L = 0, h[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0}, gh = 0, gw = 0;
    size_t buf_bytes = 0;        // one of the two rotating activation buffers, max_batch frames
    size_t ws_bytes = 0;
};
inline std::string ae_cell_error(int H, int W, int cell) {
    if (cell != 8 && cell != 16 && cell != 32) return fmt("cell=%d is not 8, 16 or 32", cell);
    const int gh = (H + cell - 1) / cell, gw = (W + cell - 1) / cell;
    if (gh > AE_MAX_GRID_SIDE || gw > AE_MAX_GRID_SIDE || gh * gw > AE_MAX_CELLS)
        return fmt("cell=%d gives a grid of %d x %d cells: at most %d cells and sides of at most %d (the box packs a byte a coordinate)",
                   cell, gh, gw, AE_MAX_CELLS, AE_MAX_GRID_SIDE);
    return std::string();
}
inline std::string ae_config_error(const fav_ae_config* c) {
    if (!c) return "null config";
    if (c->struct_size != sizeof(fav_ae_config)) return "fav_ae_config.struct_size mismatch";
    if (c->in_h < 1 || c->in_h > AE_MAX_SIDE) return fmt("in_h=%d outside [1, %d]", c->in_h, AE_MAX_SIDE);
    if (c->in_w < 1 || c->in_w > AE_MAX_SIDE) return fmt("in_w=%d outside [1, %d]", c->in_w, AE_MAX_SIDE);
    if (c->levels < 1 || c->levels > AE_MAX_LEVELS) return fmt("levels=%d outside [1, %d]", c->levels, AE_MAX_LEVELS);
    if (c->max_batch < 1) return fmt("max_batch=%d must be at least 1", c->max_batch);
    return ae_cell_error(c->in_h, c->in_w, c->cell);
}
// the geometry of a checked config.  Every activation is a matrix of bf16 rows; the two rotating buffers hold the largest
inline AeGeom ae_geometry(const fav_ae_config& c) {
    AeGeom g;
    g.L = c.levels;
    g.h[0] = c.in_h; g.w[0] = c.in_w;
    for (int l = 1; l <= g.L; ++l) { g.h[l] = (g.h[l - 1] - 1) / 2 + 1; g.w[l] = (g.w[l - 1] - 1) / 2 + 1; }
    g.gh = (c.in_h + c.cell - 1) / c.cell; g.gw = (c.in_w + c.cell - 1) / c.cell;
    const size_t n = (size_t)c.max_batch;
    size_t most = n * g.h[1] * g.w[1] * 128;                                    // the im2col matrix and enc_1's output
    for (int l = 2; l <= g.L; ++l) most = std::max(most, n * g.h[l] * g.w[l] * (size_t)ae_width(l) * 2);
    size_t rows = n * g.h[g.L] * g.w[g.L];
    for (int l = g.L; l >= 2; --l) { rows *= 4; most = std::max(most, rows * (size_t)ae_width(l - 1) * 2); }
    g.buf_bytes = (most + 255) & ~(size_t)255;
    g.ws_bytes = 2 * g.buf_bytes;
    return g;
}

// ---- host: the FAVA blob.  Header (64 bytes): magic, version 1, levels, layers = 2 levels, total size (u64); then a table of
//      (weight offset, bias offset) u64 pairs, a layer each, in the order enc_1 .. enc_L, dec_L .. dec_2, dec_1; every data
//      range 64-byte aligned.  The shapes follow from the level count, so the table only says where
struct AeLayerShape { size_t w_elems, b_elems; };
inline AeLayerShape ae_layer_shape(int levels, int k) {
    if (k == 0) return {64 * 64, 64};                                                        // enc_1: [64][64], k = (r 3 + s) 3 + c
    if (k < levels) return {(size_t)ae_width(k + 1) * 9 * ae_width(k), (size_t)ae_width(k + 1)};   // enc_{k+1}: [C][3][3][C / 2]
    const int l = 2 * levels - k;                                                            // dec_l, l = L .. 1
    if (l >= 2) return {(size_t)4 * ae_width(l - 1) * ae_width(l), (size_t)4 * ae_width(l - 1)};   // [4 C_{l-1}][C_l]
    return {12 * 64, 3};                                                                     // dec_1: [12][64], 3 biases
}
inline std::string ae_blob_error(const void* blob, size_t size, int* levels_out) {
    if (!blob || size < AE_BLOB_HEADER) return "blob too small";
    const uint8_t* p = (const uint8_t*)blob;
    uint32_t hdr[4];
    uint64_t total;
    memcpy(hdr, p, 16);
    memcpy(&total, p + 16, 8);
    if (hdr[0] != AE_BLOB_MAGIC || hdr[1] != 1u) return "not a FAVA v1 blob";
    if (hdr[2] < 1 || hdr[2] > (uint32_t)AE_MAX_LEVELS) return fmt("levels=%u outside [1, %d]", hdr[2], AE_MAX_LEVELS);
    const int L = (int)hdr[2], nl = 2 * L;
    if (hdr[3] != (uint32_t)nl) return fmt("layers=%u, but %d levels have %d layers", hdr[3], L, nl);
    if (total != size) return fmt("truncated: the header says %llu bytes, the blob has %zu", (unsigned long long)total, size);
    if ((size - AE_BLOB_HEADER) / 16 < (size_t)nl) return "truncated layer table";
    const size_t data0 = AE_BLOB_HEADER + 16 * (size_t)nl;
    for (int k = 0; k < nl; ++k) {
        uint64_t off[2];
        memcpy(off, p + AE_BLOB_HEADER + 16 * (size_t)k, 16);
        const AeLayerShape s = ae_layer_shape(L, k);
        const uint64_t bytes[2] = {s.w_elems * 2, s.b_elems * 4};
        for (int q = 0; q < 2; ++q) {
            if (off[q] % AE_BLOB_ALIGN != 0) return fmt("layer %d: %s offset %llu is not 64-byte aligned", k, q ? "bias" : "weight", (unsigned long long)off[q]);
            if (off[q] < data0 || off[q] > size || bytes[q] > size - off[q]) return fmt("layer %d: %s data out of range (truncated)", k, q ? "bias" : "weight");
        }
        for (size_t j = 0; j < s.w_elems; ++j) { uint16_t u; memcpy(&u, p + off[0] + 2 * j, 2); if ((u & 0x7F80u) == 0x7F80u) return fmt("layer %d holds a non-finite weight", k); }
        for (size_t j = 0; j < s.b_elems; ++j) { uint32_t u; memcpy(&u, p + off[1] + 4 * j, 4); if ((u & 0x7F800000u) == 0x7F800000u) return fmt("layer %d holds a non-finite bias", k); }
    }
    if (levels_out) *levels_out = L;
    return std::string();
}

// ---- host: the ranges of the decode-and-compare launch (fav_op_ae_decode_compare, fav_ae_score)
inline std::string ae_decode_dims_error(int n, int hL, int wL, int m, int H, int W, int cell, float threshold) {
    if (n < 1) return "n must be at least 1";
    if (m < 0 || m > AE_MAX_LEVELS - 1) return fmt("m=%d outside [0, %d]", m, AE_MAX_LEVELS - 1);
    if (H < 1 || H > AE_MAX_SIDE || W < 1 || W > AE_MAX_SIDE) return fmt("H=%d x W=%d: sides of 1 to %d", H, W, AE_MAX_SIDE);
    if (hL < 1 || wL < 1 || hL > AE_MAX_SIDE || wL > AE_MAX_SIDE) return fmt("h_L=%d x w_L=%d: sides of 1 to %d", hL, wL, AE_MAX_SIDE);
    if (((long long)hL << (m + 1)) < H || ((long long)wL << (m + 1)) < W)
        return fmt("h_L=%d x w_L=%d decoded %d times is smaller than the frame H=%d x W=%d", hL, wL, m + 1, H, W);
    const std::string why = ae_cell_error(H, W, cell);
    if (!why.empty()) return why;
    if ((long long)n * hL * wL * (1ll << (2 * m)) > 0x7FFFFFFFll) return "n * h_L * w_L * 4^m above 2^31 - 1";
    if ((long long)n * ((H + cell - 1) / cell) * ((W + cell - 1) / cell) > 0x7FFFFFFFll) return "n is too large for one grid";
    if (std::isnan(threshold)) return "threshold is NaN";
    return std::string();
}

// ---- device
struct AeDecodeParams {
    const uint16_t* hidden;      // [n * hL * wL * 4^m][64] bf16, 16-byte aligned
    const uint16_t* wg;          // [12][64] bf16, row (2a + b) 3 + co, 16-byte aligned
    const float* bias;           // [3]
    const void* frames;          // [n][H][W][3] u8 or fp32
    uint32_t* sse;               // [n][gh * gw]: the cell sums (the err_map buffer; ae_record_kernel turns them into means)
    uint8_t* recon;              // [n][H][W][3], or NULL
    int hL, wL, m, H, W, cell, gh, gw;
};

// the hidden row of level-1 pixel (y, x) of frame i: the coarse pixel's rows, then the Morton code of the low m bits
__device__ __forceinline__ size_t ae_row_of(int i, int y, int x, int hL, int wL, int m) {
    const size_t base = ((size_t)i * hL + (y >> m)) * wL + (x >> m);
    uint32_t d = 0;
    for (int bit = m - 1; bit >= 0; --bit) d = d * 4 + 2 * ((y >> bit) & 1) + ((x >> bit) & 1);
    return (base << (2 * m)) + d;
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void ae_decode_kernel(const AeDecodeParams p) {
    __shared__ uint32_t part_s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int cells = p.gh * p.gw;
    const int i = blockIdx.x / cells, c = blockIdx.x - i * cells, cy = c / p.gw, cx = c - cy * p.gw;
    const int s = p.cell >> 1, tiles = (s * s) >> 4;            // level-1 pixels a side; 16-row tiles: 1, 4, 16
    const int y0 = cy * s, x0 = cx * s;

    // the B fragments: weight row frow (an output column), zero for the four dead columns
    uint4 fb[2] = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
    float bias = 0.f;
    const int ab = frow / 3, co = frow - 3 * ab, oa = ab >> 1, ob = ab & 1;
    if (frow < 12) {
        fb[0] = *(const uint4*)(p.wg + frow * 64 + fq * 8);
        fb[1] = *(const uint4*)(p.wg + frow * 64 + 32 + fq * 8);
        bias = p.bias[co];
    }
    uint32_t sum = 0;
    for (int t = wave; t < tiles; t += nwaves) {               // wave-uniform
        // the A fragments: this lane's row of the tile, 16 bytes a K half; a pixel outside the level-1 grid is a zero row
        const int idx = t * 16 + frow, py = idx / s, px = idx - py * s;
        const int y1 = y0 + py, x1 = x0 + px;
        uint4 fa[2] = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
        if (2 * y1 < p.H && 2 * x1 < p.W) {
            const uint16_t* row = p.hidden + ae_row_of(i, y1, x1, p.hL, p.wL, p.m) * 64 + fq * 8;
            fa[0] = *(const uint4*)row;
            fa[1] = *(const uint4*)(row + 32);
        }
        f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            union { uint4 u; bf16x8_t v; } ua, ub;
            ua.u = fa[kk]; ub.u = fb[kk];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, acc, 0, 0, 0);
        }
        // acc[j]: row 4 fq + j of the tile, column frow
        if (frow < 12) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int id2 = t * 16 + 4 * fq + j, qy = id2 / s, qx = id2 - qy * s;
                const int oy = 2 * (y0 + qy) + oa, ox = 2 * (x0 + qx) + ob;
                if (oy < p.H && ox < p.W) {
                    const float z = __fadd_rn(acc[j], bias);
                    const float sg = __fdiv_rn(1.0f, __fadd_rn(1.0f, fav_expf(-z)));
                    const int q = (int)rintf(__fmul_rn(sg, 255.0f));
                    const size_t off = (((size_t)i * p.H + oy) * p.W + ox) * 3 + co;
                    int px8;
                    if (LAYOUT == 0) px8 = ((const uint8_t*)p.frames)[off];
                    else px8 = (int)rintf(__fmul_rn(fminf(fmaxf(fav_sanitize_px(((const float*)p.frames)[off]), 0.f), 1.f), 255.0f));
                    const int e = q - px8;
                    sum += (uint32_t)(e * e);
                    if (p.recon) p.recon[off] = (uint8_t)q;
                }
            }
        }
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) sum += __shfl_down(sum, h);
    if (lane == 0) part_s[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int w = 0; w < nwaves; ++w) total += part_s[w];
        p.sse[blockIdx.x] = total;
    }
}

struct AeRecordParams {
    float* err_map;              // [n][gh * gw]: the cell sums as uint32 on entry, the means on exit
    uint32_t* cell_sse;          // [n][gh * gw], or NULL
    int32_t* rec;                // [n] fav_ae_record, 8-byte aligned
    int H, W, cell, gh, gw;
    float threshold;
};

__global__ __launch_bounds__(AE_REC_THREADS) void ae_record_kernel(const AeRecordParams p) {
    __shared__ uint32_t sse_s[AE_MAX_CELLS];
    __shared__ float M[AE_MAX_CELLS];
    const int tid = threadIdx.x, i = blockIdx.x, cells = p.gh * p.gw;
    if (tid < cells) {
        const size_t at = (size_t)i * cells + tid;
        const uint32_t sse = ((const uint32_t*)p.err_map)[at];
        const int cy = tid / p.gw, cx = tid - cy * p.gw;
        const int inside = min(p.cell, p.H - cy * p.cell) * min(p.cell, p.W - cx * p.cell);
        const float e = (float)((double)sse / ((double)(3 * inside) * 65025.0));
        sse_s[tid] = sse;
        M[tid] = e;
        p.err_map[at] = e;
        if (p.cell_sse) p.cell_sse[at] = sse;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long total = 0;
        float peak = -INFINITY, flo = INFINITY;
        int peak_cell = -1, box = -1;
        for (int c = 0; c < cells; ++c) {
            const float v = M[c];
            total += sse_s[c];
            if (v > peak) { peak = v; peak_cell = c; }
            if (v < flo) flo = v;
        }
        const int n_above = map_box_scan(M, cells, p.gw, p.threshold, &box);
        const float mse = (float)((double)total / (3.0 * (double)p.H * (double)p.W * 65025.0));
        map_record_store(p.rec + 8 * (size_t)i, (int)(uint32_t)(total & 0xFFFFFFFFull), __float_as_int(mse), __float_as_int(peak), peak_cell,
                         __float_as_int(flo), (int)(uint32_t)(total >> 32), n_above, box);
    }
}

// ---- host: the two launches.  The arguments are checked by the caller (ae_decode_dims_error, the pointers)
inline void launch_ae_decode_compare(const void* hidden, int n, int hL, int wL, int m, const void* wg, const float* bias, const void* frames,
                                     int layout, int H, int W, int cell, float threshold, uint32_t* cell_sse, float* err_map, void* rec,
                                     uint8_t* recon, hipStream_t s) {
    AeDecodeParams p;
    p.hidden = (const uint16_t*)hidden; p.wg = (const uint16_t*)wg; p.bias = bias; p.frames = frames;
    p.sse = (uint32_t*)err_map; p.recon = recon;
    p.hL = hL; p.wL = wL; p.m = m; p.H = H; p.W = W; p.cell = cell;
    p.gh = (H + cell - 1) / cell; p.gw = (W + cell - 1) / cell;
    const int tiles = (cell / 2) * (cell / 2) / 16;
    const dim3 grid((unsigned)((long long)n * p.gh * p.gw)), block(64 * std::min(4, tiles));
    if (layout == FAV_LAYOUT_NHWC_U8) hipLaunchKernelGGL((ae_decode_kernel<0>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((ae_decode_kernel<1>), grid, block, 0, s, p);
    AeRecordParams r;
    r.err_map = err_map; r.cell_sse = cell_sse; r.rec = (int32_t*)rec;
    r.H = H; r.W = W; r.cell = cell; r.gh = p.gh; r.gw = p.gw; r.threshold = threshold;
    hipLaunchKernelGGL(ae_record_kernel, dim3(n), dim3(AE_REC_THREADS), 0, s, r);
}

}  // namespace fav
