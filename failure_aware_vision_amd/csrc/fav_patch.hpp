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

// ---- locally aware patch features (fav_op_patch_query; the contract beside fav_patch_site in fav.h) ------
//   patch_local_query_kernel<R> : one block of 256 threads a FRAME ROW (blockIdx.x = i * Hf + y), radius R.  Per channel slice
//                        of cs channels: a lane owns (cell x, eight channels) units and reads them with 16-byte loads - the
//                        2R + 1 rows of a unit, UB units at once, so four to six loads are in flight a lane - adds the samples,
//                        then the rows, and leaves v[x][j] in LDS (fp32, a row of the slice plus sixteen spare floats a cell,
//                        which break the bank conflicts of the chains and later hold the chains' sums and 1 / |a|).  A thread a
//                        (cell, chain) then runs the sixteen strided chains of the squared norm over a = the 2R + 1 neighbours
//                        of v; the chains carry on over the slices in ascending j, so the bits do not depend on the slicing.
//                        A thread a cell adds the sixteen sums up, writes the flag and 1 / |a|; the units recompute a (the same
//                        additions, so the same bits), scale, round and store eight bf16 as one 16-byte vector store.  With
//                        more than one slice the second sweep reads the rows again (from cache).  A map row is read by the
//                        2R + 1 blocks around it, from HBM by the first.  No atomics, no block waits for another.
constexpr int PQ_THREADS = 256, PQ_PAD = 16, PQ_MAX_RADIUS = 2;
constexpr int PQ_LDS_BYTES = 65536;                              // what one block may take: no opt-in, two blocks a CU
constexpr int PQ_MAX_CHAINS = PATCH_MAX_SIDE * 16 / PQ_THREADS;  // (cell, chain) pairs a thread may own

// the channels of one slice for a map Wf wide: the most whose row of v (plus the spare floats) fits, a multiple of 16
inline int patch_query_slice(int Wf, int C) { return std::min(C, (PQ_LDS_BYTES / 4 / Wf - PQ_PAD) & ~15); }

// ---- host: the one place the op's ranges live (fav_op_patch_query, fav_op_patch_score_at, fav_check_patch_site's radius)
inline std::string patch_radius_error(int radius) {
    if (radius < 0 || radius > PQ_MAX_RADIUS) return fmt("radius=%d outside [0, %d]", radius, PQ_MAX_RADIUS);
    return std::string();
}
inline std::string patch_query_error(int S, int n, int Hf, int Wf, int C, int radius) {
    if (S < 1 || S > KNN_MAX_S) return fmt("S=%d outside [1, %d]", S, KNN_MAX_S);
    const std::string map = patch_map_error(n, Hf, Wf);
    if (!map.empty()) return map;
    if (C < 64 || C > KNN_MAX_D || C % 64 != 0) return fmt("C=%d is not a multiple of 64 in [64, %d]", C, KNN_MAX_D);
    return patch_radius_error(radius);
}
inline std::string patch_site_error(const fav_patch_site* s) {
    if (!s) return "site is NULL";
    if (s->struct_size != sizeof(fav_patch_site)) return fmt("struct_size=%u is not sizeof(fav_patch_site)=%zu", s->struct_size, sizeof(fav_patch_site));
    if (s->stage < 1 || s->stage > 4) return fmt("stage=%d outside [1, 4]", s->stage);
    return patch_radius_error(s->radius);
}

struct PatchQueryParams {
    const uint16_t* maps;        // [S][n][Hf * Wf][C] bf16, 16-byte aligned
    uint16_t* q;                 // [n * Hf * Wf][C] bf16, 16-byte aligned
    int32_t* flags;              // [n * Hf * Wf]
    int S, n, Hf, Wf, C, CS;     // CS: patch_query_slice(Wf, C)
    float inv_S;
};

// a[0 .. 7] of cell x at column j of the slice: +0 plus the 2R + 1 neighbours of v in ascending dx, those outside skipped
template <int R>
__device__ __forceinline__ void pq_neighbours8(const float* v_s, int ld, int Wf, int x, int j, float* a) {
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
    for (int d = -R; d <= R; ++d) {
        const int xx = x + d;
        if (xx < 0 || xx >= Wf) continue;
        const float4 lo = *(const float4*)(v_s + xx * ld + j), hi = *(const float4*)(v_s + xx * ld + j + 4);
        const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = __fadd_rn(a[e], f[e]);
    }
}

// steps 1 and 2 for the slice [c0, c0 + cs) of frame i, row y: v[x][j] to LDS
template <int R, int UB>
__device__ __forceinline__ void pq_fill(const PatchQueryParams& p, float* v_s, int ld, int i, int y, int c0, int cs) {
    constexpr int NR = 2 * R + 1;
    const int upc = cs >> 3, units = p.Wf * upc;
    const size_t frame = (size_t)p.Hf * p.Wf * p.C, sample = (size_t)p.n * frame;
    const long long row = (long long)p.Wf * p.C;
    for (int u0 = threadIdx.x; u0 < units; u0 += PQ_THREADS * UB) {
        float acc[UB][NR][8];
        const uint16_t* src[UB];
        int at[UB];
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            const int u = u0 + k * PQ_THREADS, x = u / upc, j = (u - x * upc) * 8;
            at[k] = u < units ? x * ld + j : -1;
            src[k] = p.maps + (size_t)i * frame + ((size_t)y * p.Wf + (u < units ? x : 0)) * p.C + c0 + (u < units ? j : 0);
#pragma unroll
            for (int d = 0; d < NR; ++d)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[k][d][e] = 0.f;
        }
        for (int s = 0; s < p.S; ++s) {
            uint4 w[UB][NR];
#pragma unroll
            for (int k = 0; k < UB; ++k)
#pragma unroll
                for (int d = 0; d < NR; ++d) {
                    const int yy = y + d - R;
                    w[k][d] = make_uint4(0u, 0u, 0u, 0u);
                    if (at[k] >= 0 && yy >= 0 && yy < p.Hf) w[k][d] = *(const uint4*)(src[k] + ((long long)s * (long long)sample + (long long)(d - R) * row));
                }
#pragma unroll
            for (int k = 0; k < UB; ++k)
#pragma unroll
                for (int d = 0; d < NR; ++d) {
                    float f[8];
                    cam_unpack8(w[k][d], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[k][d][e] = __fadd_rn(acc[k][d][e], f[e]);
                }
        }
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            if (at[k] < 0) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
            for (int d = 0; d < NR; ++d) {
                const int yy = y + d - R;
                if (yy < 0 || yy >= p.Hf) continue;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = __fadd_rn(v[e], __fmul_rn(acc[k][d][e], p.inv_S));
            }
            *(float4*)(v_s + at[k]) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)(v_s + at[k] + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}

// step 4's last part for the slice [c0, c0 + cs): q = bf16(a * inv), a zero row for a degenerate cell (inv == 0)
template <int R>
__device__ __forceinline__ void pq_store(const PatchQueryParams& p, const float* v_s, int ld, int i, int y, int c0, int cs) {
    const int upc = cs >> 3, units = p.Wf * upc;
    for (int u = threadIdx.x; u < units; u += PQ_THREADS) {
        const int x = u / upc, j = (u - x * upc) * 8;
        const float inv = v_s[x * ld + p.CS];
        float a[8];
        pq_neighbours8<R>(v_s, ld, p.Wf, x, j, a);
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t lo = inv == 0.f ? 0u : (uint32_t)f32_to_bf16_bits(__fmul_rn(a[2 * e], inv));
            const uint32_t hi = inv == 0.f ? 0u : (uint32_t)f32_to_bf16_bits(__fmul_rn(a[2 * e + 1], inv));
            o[e] = (lo & 0xFFFFu) | (hi << 16);
        }
        *(uint4*)(p.q + (((size_t)i * p.Hf + y) * p.Wf + x) * p.C + c0 + j) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

template <int R, int UB>
__global__ __launch_bounds__(PQ_THREADS) void patch_local_query_kernel(const PatchQueryParams p) {
    extern __shared__ float4 pq_lds[];
    float* const v_s = (float*)pq_lds;
    const int tid = threadIdx.x, i = blockIdx.x / p.Hf, y = blockIdx.x - i * p.Hf;
    const int ld = p.CS + PQ_PAD, chains = p.Wf * 16;
    const bool one_slice = p.CS == p.C;
    float part[PQ_MAX_CHAINS];
#pragma unroll
    for (int k = 0; k < PQ_MAX_CHAINS; ++k) part[k] = 0.f;
    for (int c0 = 0; c0 < p.C; c0 += p.CS) {
        const int cs = min(p.CS, p.C - c0);
        if (c0 > 0) __syncthreads();                           // the chains of the slice before have read v
        pq_fill<R, UB>(p, v_s, ld, i, y, c0, cs);
        __syncthreads();
        // the sixteen chains of a cell, chain l over j = l, l + 16, ..: they carry on from slice to slice
#pragma unroll
        for (int k = 0; k < PQ_MAX_CHAINS; ++k) {
            const int ch = tid + k * PQ_THREADS, x = ch >> 4;
            float acc = part[k];
            for (int j = ch < chains ? (ch & 15) : cs; j < cs; j += 16) {
                float a = 0.f;
#pragma unroll
                for (int d = -R; d <= R; ++d)
                    if (x + d >= 0 && x + d < p.Wf) a = __fadd_rn(a, v_s[(x + d) * ld + j]);
                acc = __fadd_rn(acc, __fmul_rn(a, a));
            }
            part[k] = acc;
        }
    }
    // the spare floats of cell x take its sixteen sums (nobody reads them as v: a slice ends in front of them)
#pragma unroll
    for (int k = 0; k < PQ_MAX_CHAINS; ++k) {
        const int ch = tid + k * PQ_THREADS;
        if (ch < chains) v_s[(ch >> 4) * ld + p.CS + (ch & 15)] = part[k];
    }
    __syncthreads();
    for (int x = tid; x < p.Wf; x += PQ_THREADS) {
        float* const sp = v_s + x * ld + p.CS;
        float ss = sp[0];
        for (int l = 1; l < 16; ++l) ss = __fadd_rn(ss, sp[l]);
        const bool ok = ss > 0.f && ss < INFINITY;
        sp[0] = ok ? __fdiv_rn(1.0f, fav_sqrtf(ss)) : 0.f;      // as knn_query_kernel; never 0 for a cell that is ok
        p.flags[((size_t)i * p.Hf + y) * p.Wf + x] = ok ? 0 : 1;
    }
    __syncthreads();
    if (one_slice) { pq_store<R>(p, v_s, ld, i, y, 0, p.C); return; }
    for (int c0 = 0; c0 < p.C; c0 += p.CS) {
        const int cs = min(p.CS, p.C - c0);
        if (c0 > 0) __syncthreads();
        pq_fill<R, UB>(p, v_s, ld, i, y, c0, cs);
        __syncthreads();
        pq_store<R>(p, v_s, ld, i, y, c0, cs);
    }
}

}  // namespace fav
