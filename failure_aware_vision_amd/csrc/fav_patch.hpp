// fav_patch.hpp - patch-level anomaly maps behind fav_check_patch_bank, fav_set_patch_bank, fav_op_patch_score, fav_patch and
// fav_classify_patch (include/fav.h): for every cell of a frame's last feature map the distance
// to its nearest row of a bank of L2-normalised in-distribution PATCH features (PatchCore; Roth et al. 2022).  The maps
// x[S][n][HW][C] read as [S][n * HW][C] are the feat[S][n'][D] of the k-NN head, so the query kernel and the similarity GEMM are
// that head's (fav_knn.hpp), and a record is the bits of a numpy restatement (tests/patch_ref.py):
//   q = the k-NN head's, a cell a row;  sim = q . bank^T on the matrix pipe;  dist = max(2 - 2 * max_b sim, 0)
// The similarity matrix of a call (12 544 cells x 16 384 rows: 822 MB) does not fit a bounded workspace, so the bank is streamed
// in column chunks through one slab sim[M][chunk] and folded into a running nearest neighbour a cell.
// Included by fav.hip after fav_knn.hpp (the query kernel, knn_key, knn_dims_error) and fav_mapbox.hpp (the box scan, the
// record store).  Per chunk a GEMM (fav.hip's launch_conv) and a fold; then one score launch:
//
//   patch_fold_kernel  : a wave a cell, four cells a block of 256 threads - at 12 544 cells 3 136 blocks, eight a CU, thirty-two
//                        waves a CU in flight.  A lane reads 16 bytes a step (the slab's leading dimension is a multiple of 64,
//                        so a row starts on a 256-byte boundary), four steps issued ahead of their compares; it keeps the
//                        maximum of (key, -row) over its columns, six shuffle steps fold the wave's, lane 0 folds in the
//                        running state and stores it as one 8-byte vector store.  No LDS, no atomics.  Only columns below N
//                        are read: a padding row's similarity of 0 would beat every negative one.  A degenerate cell's row of
//                        the slab is never read and its state never written.
//   patch_score_kernel : one block of 256 threads a frame.  dist and nn_row of its HW cells go to LDS and to the caller's maps;
//                        one lane runs the record's serial scans in index order, then map_box_scan at the bank's threshold.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int PATCH_MAX_HW = 1024, PATCH_MAX_SIDE = 256;
constexpr int PATCH_MIN_CHUNK = 64, PATCH_MAX_CHUNK = 262144;
constexpr size_t PATCH_SLAB_BYTES = (size_t)256 << 20;       // what the default chunk lets the slab take
constexpr size_t PATCH_MAX_WS_BYTES = (size_t)1 << 30;       // what fav_set_patch_bank lets a handle's workspace take
constexpr int PATCH_FOLD_THREADS = 256, PATCH_FOLD_ROWS = PATCH_FOLD_THREADS / 64;
constexpr int PATCH_FOLD_AHEAD = 4;                          // 16-byte loads a lane has in flight
constexpr int PATCH_SCORE_THREADS = 256;
constexpr int PATCH_NO_ROW = 0x7FFFFFFF;                     // a lane, or a state, that has seen no column yet

// ---- host: the one place the ranges live (fav_check_patch_bank, fav_op_patch_score)
inline std::string patch_chunk_error(int chunk_rows) {
    if (chunk_rows == 0) return std::string();
    if (chunk_rows < PATCH_MIN_CHUNK || chunk_rows > PATCH_MAX_CHUNK || chunk_rows % 64 != 0)
        return fmt("chunk_rows=%d is neither 0 nor a multiple of 64 in [%d, %d]", chunk_rows, PATCH_MIN_CHUNK, PATCH_MAX_CHUNK);
    return std::string();
}
inline std::string patch_map_error(int n, int Hf, int Wf) {
    if (n < 1) return "n must be at least 1";
    if (Hf < 1 || Wf < 1 || Hf > PATCH_MAX_SIDE || Wf > PATCH_MAX_SIDE || Hf * Wf > PATCH_MAX_HW)
        return fmt("Hf=%d x Wf=%d: a map has 1 to %d cells and sides of at most %d (the box packs a byte a coordinate)", Hf, Wf, PATCH_MAX_HW, PATCH_MAX_SIDE);
    if ((long long)n * Hf * Wf > 0x7FFFFFFFll) return fmt("n=%d frames of %d cells are above 2^31 - 1 cells", n, Hf * Wf);
    return std::string();
}
inline std::string patch_bank_error(const fav_patch_bank* b, int D_expected) {
    if (!b) return "bank is NULL";
    if (b->struct_size != sizeof(fav_patch_bank)) return fmt("struct_size=%u is not sizeof(fav_patch_bank)=%zu", b->struct_size, sizeof(fav_patch_bank));
    const std::string dims = knn_dims_error(b->D, b->N, 1);
    if (!dims.empty()) return dims;
    if (D_expected >= 0 && b->D != D_expected) return fmt("D=%d is not the map width %d of this arch", b->D, D_expected);
    const std::string chunk = patch_chunk_error(b->chunk_rows);
    if (!chunk.empty()) return chunk;
    if (!b->rows) return "rows is NULL";
    if (std::isnan(b->threshold)) return "threshold is NaN";
    const size_t count = (size_t)b->N * b->D;
    for (size_t i = 0; i < count; ++i)
        if ((b->rows[i] & 0x7F80u) == 0x7F80u) return fmt("rows holds a non-finite value (row %zu)", i / (size_t)b->D);
    return std::string();
}

// The columns of one slab for M cells against N rows: the caller's chunk_rows when given, else the largest multiple of 128
// whose slab M * chunk * 4 fits PATCH_SLAB_BYTES, at least 128; either way at most the padded bank.  Nothing in a record
// depends on it.
inline int patch_chunk(long long M, int N, int chunk_rows) {
    const int Npad = (N + 63) & ~63;
    if (chunk_rows > 0) return std::min(chunk_rows, Npad);
    const long long fit = (long long)(PATCH_SLAB_BYTES / 4) / M / 128 * 128;
    return (int)std::min<long long>(std::max<long long>(fit, 128), Npad);
}

// The workspace of a call of M cells: [ q bf16 [M][D] | flags [M] | zero bias fp32 [chunk] | the bank's last rows as a
// zero-padded 64-row tile (only when N % 64 != 0 and the bank is not padded) | best (key, row) [M] | slab fp32 [M][chunk] ],
// every part on a 256-byte boundary.  padded_bank: the bank itself holds Npad rows (the handle's copy).
struct PatchWs {
    int Npad, chunk;
    size_t q, flags, bias, tile, best, slab, bytes;
};
inline PatchWs patch_workspace(long long M, int D, int N, int chunk_rows, bool padded_bank) {
    PatchWs w;
    w.Npad = (N + 63) & ~63;
    w.chunk = patch_chunk(M, N, chunk_rows);
    w.q = 0;
    w.flags = knn_align((size_t)M * D * 2);
    w.bias = w.flags + knn_align((size_t)M * 4);
    w.tile = w.bias + knn_align((size_t)w.chunk * 4);
    w.best = w.tile + ((N % 64 != 0 && !padded_bank) ? (size_t)64 * D * 2 : 0);
    w.slab = w.best + knn_align((size_t)M * 8);
    w.bytes = w.slab + knn_align((size_t)M * w.chunk * 4);
    return w;
}

// ---- device
struct PatchFoldParams {
    const float* sim;            // [M][ld] fp32: this chunk's slab, columns below `cols` valid
    const int32_t* flags;        // [M]
    uint2* best;                 // [M] (key, row)
    long long M;
    int cols, ld, row0, first;   // row0: the bank row of column 0; first: this chunk initialises the state
};

// (key, row) a beats (okey, orow): the maximum of (sim, -row); a side that has seen no column loses
__device__ __forceinline__ void patch_take(uint32_t& key, int& row, uint32_t okey, int orow) {
    if (orow != PATCH_NO_ROW && (row == PATCH_NO_ROW || okey > key || (okey == key && orow < row))) { key = okey; row = orow; }
}

__global__ __launch_bounds__(PATCH_FOLD_THREADS) void patch_fold_kernel(const PatchFoldParams p) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PATCH_FOLD_ROWS + (threadIdx.x >> 6);
    if (r >= p.M || p.flags[r] != 0) return;              // the whole wave takes this branch
    const float* const row = p.sim + (size_t)r * p.ld;
    const int cols = p.cols;
    uint32_t key = 0;
    int best = PATCH_NO_ROW;
    for (int b0 = lane * 4; b0 < cols; b0 += 64 * 4 * PATCH_FOLD_AHEAD) {
        float4 v[PATCH_FOLD_AHEAD];
#pragma unroll
        for (int q = 0; q < PATCH_FOLD_AHEAD; ++q) {
            const int b = b0 + q * 256;
            v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b < cols) v[q] = *(const float4*)(row + b);               // ld is a multiple of 64: the row holds whole quads
        }
#pragma unroll
        for (int q = 0; q < PATCH_FOLD_AHEAD; ++q) {
            const float e[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = b0 + q * 256 + j;
                const uint32_t k = knn_key(e[j]);
                if (b < cols && (best == PATCH_NO_ROW || k > key)) { key = k; best = b; }   // b ascends: ties keep the lower row
            }
        }
    }
    if (best != PATCH_NO_ROW) best += p.row0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t okey = (uint32_t)__shfl_xor((int)key, off);
        const int orow = __shfl_xor(best, off);
        patch_take(key, best, okey, orow);
    }
    if (lane == 0) {
        if (!p.first) {
            const uint2 old = p.best[r];
            patch_take(key, best, old.x, (int)old.y);
        }
        p.best[r] = make_uint2(key, (uint32_t)best);
    }
}

struct PatchScoreParams {
    const uint2* best;           // [n * HW] (key, row); a degenerate cell's is unwritten
    const int32_t* flags;        // [n * HW]
    float* dist;                 // [n][HW]
    int32_t* row;                // [n][HW] or NULL
    int32_t* rec;                // [n] fav_patch_record, 8-byte aligned
    int HW, Wf;
    float threshold, inv_HW;
};

__global__ __launch_bounds__(PATCH_SCORE_THREADS) void patch_score_kernel(const PatchScoreParams p) {
    __shared__ float d_s[PATCH_MAX_HW];
    __shared__ int r_s[PATCH_MAX_HW];
    const int tid = threadIdx.x, HW = p.HW;
    const size_t base = (size_t)blockIdx.x * HW;
    // 3: the distance of a cell, from its nearest row's similarity
    for (int c = tid; c < HW; c += PATCH_SCORE_THREADS) {
        float d = __int_as_float(0x7FC00000);
        int row = -1;
        if (p.flags[base + c] == 0) {
            const uint2 b = p.best[base + c];
            d = fmaxf(__fsub_rn(2.0f, __fmul_rn(2.0f, knn_unkey(b.x))), 0.0f);
            row = (int)b.y;
        }
        d_s[c] = d; r_s[c] = row;
        p.dist[base + c] = d;
        if (p.row) p.row[base + c] = row;
    }
    __syncthreads();
    // 4: the record, by one lane: serial scans in index order
    if (tid == 0) {
        float sum = 0.f, peak = -INFINITY, flo = INFINITY;
        int n_deg = 0, peak_cell = -1, box;
        for (int c = 0; c < HW; ++c) {
            const float v = d_s[c];
            if (r_s[c] < 0) ++n_deg;
            sum = __fadd_rn(sum, v);
            if (v > peak) { peak = v; peak_cell = c; }
            if (v < flo) flo = v;
        }
        const int n_above = map_box_scan(d_s, HW, p.Wf, p.threshold, &box);
        map_record_store(p.rec + 8 * (size_t)blockIdx.x, n_deg, __float_as_int(__fmul_rn(sum, p.inv_HW)), __float_as_int(peak), peak_cell,
                         __float_as_int(flo), peak_cell >= 0 ? r_s[peak_cell] : -1, n_above, box);
    }
}

}  // namespace fav
