// fav_drift.hpp - window-level drift detection behind fav_check_drift_ref, fav_set_drift, fav_op_drift_test and
// fav_classify_drift (include/fav.h): a two-sample permutation test on the energy distance
// (Szekely & Rizzo; the test of Rabanser et al. 2019) between a held-out reference of R L2-normalised features and the n frames
// of one call.  The contract beside fav_drift_record fixes every operation, so a record is the bits of a numpy restatement
// (tests/drift_ref.py): the pairwise distances of the pool [reference | window] are quantised to integers, 2^-20 a step, and
// from there on every sum is an exact integer and every comparison a 128-bit one.
// Included by fav.hip after fav_knn.hpp.  The launches of one call:
//
//   knn_query_kernel      : fav_knn.hpp's, as it is - the window's rows, written straight behind the reference in the pool
//   the GEMM              : fav.hip's launch_conv as a 1x1 convolution, fp32 output, a zero bias: pool rows against pool rows.
//                           The op computes the whole matrix; a handle computed the reference's block once, in the setter
//   drift_quant_kernel    : one block a pool row i of its block of rows, threads over j <= i: the distance, quantised, into
//                           both triangles of U.  Only G[i][j] with j <= i is ever read
//   drift_rowsum_kernel   : r[i] = sum_j U[i][j], one wave a row
//   drift_perm_kernel     : one block of 1024 threads a permutation, and one more for the observed grouping.  Philox keys,
//                           a bitonic sort in LDS, the n smallest as an ascending index list (ascending: the lanes of a wave
//                           then gather from neighbouring columns of one row of U), the gather-sum over B x B, the n row sums
//   drift_final_kernel    : one block: the exceedance count in 128-bit integers, one thread's float64 arithmetic, the record
//
// A call with a degenerate frame: the blocks of the permutation kernel return before they compute anything and the final
// kernel writes the record of step 1; nothing that a later call reads has been changed.
#pragma once

namespace fav {

constexpr int DRIFT_MAX_D = 4096, DRIFT_MAX_R = 2048, DRIFT_MAX_N = 1024, DRIFT_MAX_P = 9999, DRIFT_MAX_S = 4096;
constexpr int DRIFT_PERM_THREADS = 1024, DRIFT_PERM_WAVES = DRIFT_PERM_THREADS / 64;
constexpr int DRIFT_SORT_MAX = 4096;                     // the next power of two above R + n <= 3072
constexpr int DRIFT_FINAL_THREADS = 256;

// ---- host: the one place the ranges live (fav_check_drift_ref).  n: a call's frames, or NULL: the reference alone
inline std::string drift_dims_error(int D, int R, int n_perm, float alpha, const int* n) {
    if (D < 64 || D > DRIFT_MAX_D || D % 64 != 0) return fmt("D=%d is not a multiple of 64 in [64, %d]", D, DRIFT_MAX_D);
    if (R < 2 || R > DRIFT_MAX_R) return fmt("R=%d outside [2, %d]", R, DRIFT_MAX_R);
    if (n_perm < 1 || n_perm > DRIFT_MAX_P) return fmt("n_perm=%d outside [1, %d]", n_perm, DRIFT_MAX_P);
    if (!(alpha >= 0.f && alpha <= 1.f)) return fmt("alpha=%g outside [0, 1]", (double)alpha);
    if (n && (*n < 2 || *n > DRIFT_MAX_N)) return fmt("n=%d outside [2, %d]", *n, DRIFT_MAX_N);
    return std::string();
}
inline std::string drift_ref_error(const fav_drift_ref* b, int D_expected) {
    if (!b) return "ref is NULL";
    if (b->struct_size != sizeof(fav_drift_ref)) return fmt("struct_size=%u is not sizeof(fav_drift_ref)=%zu", b->struct_size, sizeof(fav_drift_ref));
    const std::string dims = drift_dims_error(b->D, b->R, b->n_perm, b->alpha, nullptr);
    if (!dims.empty()) return dims;
    if (D_expected >= 0 && b->D != D_expected) return fmt("D=%d is not the feature width %d of this arch", b->D, D_expected);
    if (!b->rows) return "rows is NULL";
    for (int r = 0; r < b->R; ++r) {
        double ss = 0.0;
        for (int j = 0; j < b->D; ++j) {
            const uint16_t v = b->rows[(size_t)r * b->D + j];
            if ((v & 0x7F80u) == 0x7F80u) return fmt("rows holds a non-finite value (row %d)", r);
            const uint32_t u = (uint32_t)v << 16;
            float f;
            memcpy(&f, &u, 4);
            ss += (double)f * (double)f;
        }
        if (!(ss >= 0.5 && ss <= 2.0)) return fmt("rows: the squared norm %.9g of row %d lies outside [0.5, 2]", ss, r);
    }
    return std::string();
}

// The workspace for calls of up to nmax frames: [ pool bf16 [ld][D]: the reference, the window's rows behind it, zero rows up
// to ld | flags [nmax] | zero bias fp32 [ld] | the reference's diagonal fp32 [ld] | G fp32 [rows][ld] | U uint32 [R + nmax][ld]
// | r int64 [R + nmax] | sums int64 [P + 1][2], the last pair the observed grouping's ], every part on a 256-byte boundary.
// cached_ref: the reference's block of U is there already (a handle), so G holds the window's rows only.
struct DriftWs {
    int ld;
    size_t pool, flags, bias, diag, G, U, r, sums, bytes;
};
inline DriftWs drift_workspace(long long nmax, int D, int R, int P, bool cached_ref) {
    DriftWs w;
    w.ld = (int)((R + nmax + 63) & ~63ll);
    const size_t pool_rows = (size_t)(R + nmax);
    w.pool = 0;
    w.flags = knn_align((size_t)w.ld * D * 2);
    w.bias = w.flags + knn_align((size_t)nmax * 4);
    w.diag = w.bias + knn_align((size_t)w.ld * 4);
    w.G = w.diag + knn_align((size_t)w.ld * 4);
    w.U = w.G + knn_align((cached_ref ? (size_t)nmax : pool_rows) * w.ld * 4);
    w.r = w.U + knn_align(pool_rows * w.ld * 4);
    w.sums = w.r + knn_align(pool_rows * 8);
    w.bytes = w.sums + knn_align((size_t)(P + 1) * 16);
    return w;
}

struct DriftQuantParams {
    const float* G;              // [rows][ldg]: pool rows row0 .. row0 + rows - 1 against the pool
    float* diag;                 // [>= row0 + rows] G[k][k]: read for k < row0, written for the block's own rows
    uint32_t* U;                 // [Np][ldu]
    int row0, rows, ldg, ldu;
};

// 4: the distance of pool rows i and j <= i, in steps of 2^-20
__global__ __launch_bounds__(256) void drift_quant_kernel(const DriftQuantParams p) {
    const int i = p.row0 + (int)blockIdx.x;
    const float* const row = p.G + (size_t)blockIdx.x * p.ldg;
    const float gii = row[i];
    for (int j = threadIdx.x; j <= i; j += 256) {
        if (j == i) {
            p.U[(size_t)i * p.ldu + i] = 0u;
            p.diag[i] = gii;
            continue;
        }
        const float gjj = j >= p.row0 ? p.G[(size_t)(j - p.row0) * p.ldg + j] : p.diag[j];
        const float d2 = fmaxf(__fsub_rn(__fadd_rn(gii, gjj), __fmul_rn(2.0f, row[j])), 0.0f);
        const uint32_t u = (uint32_t)rintf(__fmul_rn(fav_sqrtf(d2), 1048576.0f));
        p.U[(size_t)i * p.ldu + j] = u;
        p.U[(size_t)j * p.ldu + i] = u;
    }
}

__device__ __forceinline__ long long drift_shfl_xor(long long v, int off) {
    const int lo = __shfl_xor((int)(v & 0xFFFFFFFFll), off), hi = __shfl_xor((int)(v >> 32), off);
    return ((long long)hi << 32) | (long long)(uint32_t)lo;
}
__device__ __forceinline__ long long drift_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += drift_shfl_xor(v, off);
    return v;
}

// 5: r[i], one wave a row
__global__ __launch_bounds__(256) void drift_rowsum_kernel(const uint32_t* U, long long* r, int Np, int ld) {
    const int i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Np) return;                                     // a whole wave
    const uint32_t* const row = U + (size_t)i * ld;
    long long acc = 0;
    for (int j = lane; j < Np; j += 64) acc += (long long)row[j];
    acc = drift_wave_sum(acc);
    if (lane == 0) r[i] = acc;
}

struct DriftPermParams {
    const uint32_t* U;           // [Np][ld]
    const long long* r;          // [Np]
    const int32_t* flags;        // [n]
    long long* sums;             // [P + 1][2]: (S_BB, S_AB); pair P is the observed grouping's
    long long* user_sums;        // [P][2] or NULL
    int R, n, Np, ld, P, sort_n; // sort_n: the power of two the keys are padded to
    uint32_t seed_lo, seed_hi;
};

__global__ __launch_bounds__(DRIFT_PERM_THREADS) void drift_perm_kernel(const DriftPermParams p) {
    __shared__ unsigned long long keys[DRIFT_SORT_MAX];
    __shared__ int B[DRIFT_MAX_N];
    __shared__ unsigned char member[DRIFT_MAX_R + DRIFT_MAX_N];
    __shared__ int w_cnt[DRIFT_PERM_WAVES];
    __shared__ long long w_bb[DRIFT_PERM_WAVES], w_r[DRIFT_PERM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, perm = blockIdx.x;
    const int n = p.n, Np = p.Np;
    int bad = 0;
    for (int a = tid; a < n; a += DRIFT_PERM_THREADS) bad |= p.flags[a];
    if (__syncthreads_or(bad)) return;                        // 1: the test is not run
    if (perm == p.P) {
        for (int a = tid; a < n; a += DRIFT_PERM_THREADS) B[a] = p.R + a;
    } else {
        // 6: the keys, sorted ascending
        const int sort_n = p.sort_n;
        for (int i = tid; i < sort_n; i += DRIFT_PERM_THREADS) {
            unsigned long long key = ~0ull;
            if (i < Np) key = ((unsigned long long)philox4x32_10(make_uint4((uint32_t)i, (uint32_t)perm, 0u, 0x5F17u), p.seed_lo, p.seed_hi).x << 32) | (uint32_t)i;
            keys[i] = key;
        }
        for (int i = tid; i < Np; i += DRIFT_PERM_THREADS) member[i] = 0;
        __syncthreads();
        for (int k = 2; k <= sort_n; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (sort_n >> 1); t += DRIFT_PERM_THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const unsigned long long a = keys[lo], b = keys[hi];
                    if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
                }
                __syncthreads();
            }
        // the n smallest as a set, then as an ascending list: a thread owns a run of `per` pool indices
        for (int a = tid; a < n; a += DRIFT_PERM_THREADS) member[(uint32_t)keys[a]] = 1;
        __syncthreads();
        const int per = (Np + DRIFT_PERM_THREADS - 1) / DRIFT_PERM_THREADS;
        const int i0 = tid * per, i1 = min(Np, i0 + per);
        int c = 0;
        for (int i = i0; i < i1; ++i) c += member[i];
        int x = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) w_cnt[wave] = x;
        __syncthreads();
        int pos = x - c;
        for (int w = 0; w < wave; ++w) pos += w_cnt[w];
        for (int i = i0; i < i1; ++i)
            if (member[i]) B[pos++] = i;
    }
    __syncthreads();
    // 5: S_BB, a wave a row of the group, its lanes over the columns below it; a 32-bit partial holds at most 16 terms
    long long bb = 0;
    for (int a = 1 + wave; a < n; a += DRIFT_PERM_WAVES) {
        const uint32_t* const row = p.U + (size_t)B[a] * p.ld;
        uint32_t part = 0;
        for (int b = lane; b < a; b += 64) part += row[B[b]];
        bb += (long long)part;
    }
    long long sr = 0;
    for (int a = tid; a < n; a += DRIFT_PERM_THREADS) sr += p.r[B[a]];
    bb = drift_wave_sum(bb);
    sr = drift_wave_sum(sr);
    if (lane == 0) { w_bb[wave] = bb; w_r[wave] = sr; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DRIFT_PERM_WAVES; ++w) { bb += w_bb[w]; sr += w_r[w]; }
        const long long ab = sr - 2 * bb;
        p.sums[2 * (size_t)perm] = bb;
        p.sums[2 * (size_t)perm + 1] = ab;
        if (p.user_sums && perm < p.P) {
            p.user_sums[2 * (size_t)perm] = bb;
            p.user_sums[2 * (size_t)perm + 1] = ab;
        }
    }
}

struct DriftFinalParams {
    const long long* r;          // [Np]
    const long long* sums;       // [P + 1][2]
    const int32_t* flags;        // [n]
    unsigned long long* rec;     // one fav_drift_record as six 8-byte words
    int R, n, Np, P;
    float alpha;
};

// the sum of v over the block's DRIFT_FINAL_THREADS threads, in every thread
__device__ __forceinline__ long long drift_block_sum(long long v, long long* lds) {
    v = drift_wave_sum(v);
    __syncthreads();                                         // lds may still be read from the last call
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
    for (int w = 0; w < DRIFT_FINAL_THREADS / 64; ++w) s += lds[w];
    return s;
}

// 7: T = S_AB (R n) - S_AA n^2 - S_BB R^2 - below 2^68 in magnitude
__device__ __forceinline__ __int128 drift_T(long long ab, long long aa, long long bb, long long R, long long n) {
    return (__int128)ab * (__int128)(R * n) - (__int128)aa * (__int128)(n * n) - (__int128)bb * (__int128)(R * R);
}

__global__ __launch_bounds__(DRIFT_FINAL_THREADS) void drift_final_kernel(const DriftFinalParams p) {
    __shared__ long long lds[DRIFT_FINAL_THREADS / 64];
    const int tid = threadIdx.x;
    long long v = 0;
    for (int a = tid; a < p.n; a += DRIFT_FINAL_THREADS) v += p.flags[a] != 0 ? 1 : 0;
    const long long n_bad = drift_block_sum(v, lds);
    if (n_bad != 0) {                                        // 1: the whole block takes this branch
        if (tid == 0) {
            p.rec[0] = 0x7FF8000000000000ull;
            p.rec[1] = p.rec[2] = p.rec[3] = 0ull;
            p.rec[4] = 0x7FC00000ull | (0xFFFFFFFFull << 32);
            p.rec[5] = 1ull | ((unsigned long long)n_bad << 32);
        }
        return;
    }
    v = 0;
    for (int i = tid; i < p.Np; i += DRIFT_FINAL_THREADS) v += p.r[i];
    const long long s_tot = drift_block_sum(v, lds) / 2;
    const long long R = p.R, n = p.n;
    const long long bb = p.sums[2 * (size_t)p.P], ab = p.sums[2 * (size_t)p.P + 1], aa = s_tot - bb - ab;
    const __int128 t_obs = drift_T(ab, aa, bb, R, n);
    v = 0;
    for (int q = tid; q < p.P; q += DRIFT_FINAL_THREADS) {
        const long long bq = p.sums[2 * (size_t)q], aq = p.sums[2 * (size_t)q + 1];
        v += drift_T(aq, s_tot - bq - aq, bq, R, n) >= t_obs ? 1 : 0;
    }
    const long long n_exceed = drift_block_sum(v, lds);
    if (tid == 0) {
        // 8: float64, every operation rounded on its own
        const double e_ab = __ddiv_rn(__dmul_rn(2.0, (double)ab), (double)(R * n));
        const double e_aa = __ddiv_rn(__dmul_rn(2.0, (double)aa), (double)(R * R));
        const double e_bb = __ddiv_rn(__dmul_rn(2.0, (double)bb), (double)(n * n));
        const double E = __dmul_rn(__dsub_rn(__dsub_rn(e_ab, e_aa), e_bb), 0x1p-20);
        const float pv = (float)__ddiv_rn((double)(1 + n_exceed), (double)(p.P + 1));
        const uint32_t drift = pv <= p.alpha ? 1u : 0u;
        p.rec[0] = (unsigned long long)__double_as_longlong(E);
        p.rec[1] = (unsigned long long)ab;
        p.rec[2] = (unsigned long long)aa;
        p.rec[3] = (unsigned long long)bb;
        p.rec[4] = (unsigned long long)__float_as_uint(pv) | ((unsigned long long)(uint32_t)n_exceed << 32);
        p.rec[5] = (unsigned long long)drift | (0ull << 32);
    }
}

}  // namespace fav
