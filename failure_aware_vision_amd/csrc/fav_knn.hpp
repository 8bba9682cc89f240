// fav_knn.hpp - nearest-neighbour OOD scoring behind fav_check_knn_bank, fav_set_knn, fav_op_knn_score and fav_classify_knn
// (include/fav.h): a frame's distance to its k-th nearest row of a bank of L2-normalised
// in-distribution features (deep nearest neighbours; Sun et al. 2022).  The contract beside fav_knn_record fixes every
// operation, so a record is the bits of a numpy restatement (tests/knn_ref.py):
//   fbar = (sum_s feat[s]) * fp32(1 / S);  q = bf16(fbar / |fbar|);  sim = q . bank^T on the matrix pipe;
//   kth_dist = max(2 - 2 * (k-th largest sim), 0)
// Included by fav.hip after fav_ood.hpp.  Three launches:
//
//   knn_query_kernel  : one block of 256 threads a frame.  fbar goes to LDS, sixteen threads run the sixteen strided chains
//                       of the squared norm, one thread adds them up in index order, all of them scale and round.  Writes q
//                       bf16 [n][D] and one flag a frame (1: degenerate - a zero row of q then, so that the GEMM reads
//                       nothing wild).
//   the GEMM          : fav.hip's launch_conv as a 1x1 convolution over n one-pixel frames, fp32 output, a zero bias: the
//                       production accumulator, K never split.  It wants whole 64-row tiles of the bank: a bank of N rows is
//                       read in place up to its last multiple of 64, the rest goes through a zero-padded 64-row tile in the
//                       workspace (the handle's own copy is padded once, by the setter).
//   knn_select_kernel : one block of 1024 threads a frame (a call of 256 frames is one block a CU: sixteen waves keep enough
//                       loads in flight, four did not).  An exact radix select of the k-th largest of the N similarities
//                       of its row: fp32 to order-preserving uint32 keys, four 8-bit digits from the top, a 256-bin LDS
//                       histogram a pass over the keys that share the digits found so far.  The first pass also finds the
//                       lexicographic maximum of (sim, -row).  Only columns below N are read: a padding row's similarity of
//                       0 would beat every negative one.  A degenerate frame's row of similarities is never read.
#pragma once

namespace fav {

constexpr int KNN_MAX_D = 4096, KNN_MAX_N = 262144, KNN_MAX_K = 256, KNN_MAX_S = 4096;
constexpr int KNN_THREADS = 256;                         // the query kernel's block
constexpr int KNN_SEL_THREADS = 1024, KNN_SEL_WAVES = KNN_SEL_THREADS / 64;
constexpr size_t KNN_MAX_WS_BYTES = (size_t)1 << 30;     // what fav_set_knn lets a handle's workspace take

// ---- host: the one place the bank's ranges live (fav_check_knn_bank).  D_expected < 0: any width in range
inline std::string knn_dims_error(int D, int N, int k) {
    if (D < 64 || D > KNN_MAX_D || D % 64 != 0) return fmt("D=%d is not a multiple of 64 in [64, %d]", D, KNN_MAX_D);
    if (N < 1 || N > KNN_MAX_N) return fmt("N=%d outside [1, %d]", N, KNN_MAX_N);
    if (k < 1 || k > std::min(N, KNN_MAX_K)) return fmt("k=%d outside [1, min(N, %d)=%d]", k, KNN_MAX_K, std::min(N, KNN_MAX_K));
    return std::string();
}
inline std::string knn_bank_error(const fav_knn_bank* b, int D_expected) {
    if (!b) return "bank is NULL";
    if (b->struct_size != sizeof(fav_knn_bank)) return fmt("struct_size=%u is not sizeof(fav_knn_bank)=%zu", b->struct_size, sizeof(fav_knn_bank));
    const std::string dims = knn_dims_error(b->D, b->N, b->k);
    if (!dims.empty()) return dims;
    if (D_expected >= 0 && b->D != D_expected) return fmt("D=%d is not the feature width %d of this arch", b->D, D_expected);
    if (!b->rows) return "rows is NULL";
    if (std::isnan(b->threshold)) return "threshold is NaN";
    const size_t count = (size_t)b->N * b->D;
    for (size_t i = 0; i < count; ++i)
        if ((b->rows[i] & 0x7F80u) == 0x7F80u) return fmt("rows holds a non-finite value (row %zu)", i / (size_t)b->D);
    if (b->class_id)
        for (int r = 0; r < b->N; ++r)
            if (b->class_id[r] < -1) return fmt("class_id[%d]=%d is below -1", r, b->class_id[r]);
    return std::string();
}

// The workspace of a call of n frames: [ q bf16 [n][D] | flags [n] | zero bias fp32 [Npad] | the bank's last rows as a
// zero-padded 64-row tile (only when N % 64 != 0 and the bank is not padded) | sim fp32 [n][Npad] ], every part on a
// 256-byte boundary.  padded_bank: the bank itself holds Npad rows (the handle's copy).
struct KnnWs {
    int Npad;
    size_t q, flags, bias, tile, sim, bytes;
};
inline size_t knn_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline KnnWs knn_workspace(long long n, int D, int N, bool padded_bank) {
    KnnWs w;
    w.Npad = (N + 63) & ~63;
    w.q = 0;
    w.flags = knn_align((size_t)n * D * 2);
    w.bias = w.flags + knn_align((size_t)n * 4);
    w.tile = w.bias + knn_align((size_t)w.Npad * 4);
    w.sim = w.tile + ((N % 64 != 0 && !padded_bank) ? (size_t)64 * D * 2 : 0);
    w.bytes = w.sim + knn_align((size_t)n * w.Npad * 4);
    return w;
}

struct KnnQueryParams {
    const uint16_t* feat;        // [S][n][D] bf16
    uint16_t* q;                 // [n][D] bf16
    int32_t* flags;              // [n]
    int S, n, D;
    float inv_S;
};

__global__ __launch_bounds__(KNN_THREADS) void knn_query_kernel(const KnnQueryParams p) {
    __shared__ float fbar[KNN_MAX_D];
    __shared__ float part[16];
    __shared__ float s_inv;
    __shared__ int s_bad;
    const int tid = threadIdx.x, D = p.D, i = blockIdx.x;
    // 1: fbar = (sum_s feat[s]) * fp32(1 / S), s ascending
    for (int j = tid; j < D; j += KNN_THREADS) {
        float sum = 0.f;
        for (int s = 0; s < p.S; ++s) sum = __fadd_rn(sum, bf16_bits_to_f32(p.feat[((size_t)s * p.n + i) * D + j]));
        fbar[j] = __fmul_rn(sum, p.inv_S);
    }
    __syncthreads();
    // 2: sixteen chains over j = l, l + 16, ..; then their sum in index order
    if (tid < 16) {
        float acc = 0.f;
        for (int j = tid; j < D; j += 16) acc = __fadd_rn(acc, __fmul_rn(fbar[j], fbar[j]));
        part[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        float ss = part[0];
        for (int l = 1; l < 16; ++l) ss = __fadd_rn(ss, part[l]);
        // 3, 7: a degenerate frame has no direction
        const bool ok = ss > 0.f && ss < INFINITY;
        s_bad = ok ? 0 : 1;
        s_inv = ok ? __fdiv_rn(1.0f, fav_sqrtf(ss)) : 0.f;    // both correctly rounded (fav_sqrtf: __fsqrt_rn is not, here)
        p.flags[i] = ok ? 0 : 1;
    }
    __syncthreads();
    const float inv = s_inv;
    const bool bad = s_bad != 0;
    for (int j = tid; j < D; j += KNN_THREADS)
        p.q[(size_t)i * D + j] = bad ? (uint16_t)0 : (uint16_t)f32_to_bf16_bits(__fmul_rn(fbar[j], inv));
}

struct KnnSelectParams {
    const float* sim;            // [n][ld] fp32, columns below N valid
    const int32_t* flags;        // [n]
    const int32_t* cls;          // [N] or NULL
    int32_t* rec;                // [n] fav_knn_record, 8-byte aligned
    int N, ld, k;
    float threshold;
};

// fp32 -> uint32 keys in the order of the values (no NaN reaches them; -0 < +0, and the contract's + 0.0f rules -0 out)
__device__ __forceinline__ uint32_t knn_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unkey(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

__global__ __launch_bounds__(KNN_SEL_THREADS) void knn_select_kernel(const KnnSelectParams p) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t w_key[KNN_SEL_WAVES];
    __shared__ int w_row[KNN_SEL_WAVES];
    __shared__ uint32_t s_prefix;
    __shared__ int s_want;
    const int tid = threadIdx.x, i = blockIdx.x, N = p.N;
    int2* const out = (int2*)(p.rec + 6 * (size_t)i);
    if (p.flags[i] != 0) {          // 7: the whole block takes this branch
        if (tid == 0) {
            const int nan = 0x7FC00000;
            out[0] = make_int2(nan, nan);
            out[1] = make_int2(nan, -1);
            out[2] = make_int2(-1, 1);
        }
        return;
    }
    const float* const row = p.sim + (size_t)i * p.ld;
    uint32_t prefix = 0;            // the digits of the k-th largest key found so far
    int want = p.k;                 // its rank among the keys that share them, from the top
    uint32_t best_key = 0;
    int best_row = 0x7FFFFFFF;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        // a thread adds a run of equal digits at once: most rows of a bank share their sign and high exponent bits
        int run_bin = -1;
        uint32_t run = 0;
        for (int b0 = tid * 4; b0 < N; b0 += KNN_SEL_THREADS * 4) {          // ld is a multiple of 64: the row holds whole quads
            const float4 v4 = *(const float4*)(row + b0);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = b0 + e;
                if (b >= N) break;                                        // padding columns never take part
                const uint32_t key = knn_key(v[e]);
                if (pass == 0 && (key > best_key || best_row == 0x7FFFFFFF)) { best_key = key; best_row = b; }   // b ascends: ties keep the lower row
                if ((key & mask) != prefix) continue;
                const int bin = (int)((key >> shift) & 0xFFu);
                if (bin != run_bin) {
                    if (run) atomicAdd(&hist[run_bin], run);
                    run_bin = bin; run = 0;
                }
                ++run;
            }
        }
        if (run) atomicAdd(&hist[run_bin], run);
        __syncthreads();
        if (tid == 0) {
            int bin = 255, left = want;
            for (; bin > 0; --bin) {                                      // from the top: the bin that holds rank `left`
                const int c = (int)hist[bin];
                if (c >= left) break;
                left -= c;
            }
            s_prefix = prefix | ((uint32_t)bin << shift);
            s_want = left;
        }
        __syncthreads();
        prefix = s_prefix;
        want = s_want;
    }
    // 5: the lexicographic maximum of (sim, -row): the wave's, then the block's
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)best_key, off);
        const int orow = __shfl_xor(best_row, off);
        if (orow != 0x7FFFFFFF && (best_row == 0x7FFFFFFF || ok > best_key || (ok == best_key && orow < best_row))) { best_key = ok; best_row = orow; }
    }
    if ((tid & 63) == 0) { w_key[tid >> 6] = best_key; w_row[tid >> 6] = best_row; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < KNN_SEL_WAVES; ++w) {
            const uint32_t ok = w_key[w];
            const int orow = w_row[w];
            if (orow != 0x7FFFFFFF && (best_row == 0x7FFFFFFF || ok > best_key || (ok == best_key && orow < best_row))) { best_key = ok; best_row = orow; }
        }
        // 5, 6: the record, as three 8-byte stores
        const float kth_sim = knn_unkey(prefix), nn_sim = knn_unkey(best_key);
        const float kth_dist = fmaxf(__fsub_rn(2.0f, __fmul_rn(2.0f, kth_sim)), 0.0f);
        const int nn_class = p.cls ? p.cls[best_row] : -1;
        out[0] = make_int2(__float_as_int(kth_dist), __float_as_int(kth_sim));
        out[1] = make_int2(__float_as_int(nn_sim), best_row);
        out[2] = make_int2(nn_class, !(kth_dist <= p.threshold) ? 1 : 0);
    }
}

}  // namespace fav
