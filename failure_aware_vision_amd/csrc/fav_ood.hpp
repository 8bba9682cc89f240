// fav_ood.hpp - feature-space OOD scoring behind fav_check_ood_model, fav_set_ood, fav_op_ood_score and fav_classify_ood
// (include/fav.h): the Mahalanobis distance of a frame's pooled features to a set of class
// means, as a whitening projection P and projected means M.  The contract fixes every operation - fp32, one rounding per
// product and per sum, sums in index order - so the result is the bits of a numpy restatement (tests/ood_ref.py):
//   fbar = (sum_s feat[s]) * fp32(1 / S);  x = fbar - mu;  g[r] = sum_j P[r][j] * x[j];  d[c] = sum_r (g[r] - M[c][r])^2
// Included by fav.hip after fav_route.hpp (fmt).
//
//   ood_score_kernel<FPB> : one block of 1024 threads per FPB frames, ONE launch and no global workspace.  x, then g, stay in
//                           LDS, the FPB frames' values of an index side by side (one LDS read serves all of them).  Every
//                           chain is serial in its own index, so the parallelism is across outputs: a thread owns a column
//                           r of the projection (then a row c of the means) for the block's FPB frames, reads Pt[j][r]
//                           (Mt[r][c]) coalesced along the column and x[j] (g[r]) as an LDS broadcast.  A chain step is a
//                           load, a product and a sum, so the kernel lives on loads in flight: sixteen waves a block, the
//                           loads of eight steps issued ahead of their chain.  The minimum is the lexicographic minimum of
//                           (d, row) over the rows a thread met in ascending order, so ties go to the lowest row and a NaN
//                           never wins, as in the serial scan of the contract.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int OOD_MAX_D = 4096, OOD_MAX_K = 2048, OOD_MAX_R = 4096, OOD_MAX_S = 4096;
constexpr int OOD_LDS_BYTES = 64 * 1024;                 // the dynamic LDS a launch may ask for without raising the limit
constexpr int OOD_THREADS = 1024, OOD_WAVES = OOD_THREADS / 64;

// ---- host: the one place the model's ranges live (fav_check_ood_model).  D_expected < 0: any width in range
inline bool ood_all_finite(const float* v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
inline std::string ood_dims_error(int D, int k, int R) {
    if (D < 16 || D > OOD_MAX_D || D % 16 != 0) return fmt("D=%d is not a multiple of 16 in [16, %d]", D, OOD_MAX_D);
    if (k < 1 || k > OOD_MAX_K) return fmt("k=%d outside [1, %d]", k, OOD_MAX_K);
    if (R < 1 || R > OOD_MAX_R) return fmt("R=%d outside [1, %d]", R, OOD_MAX_R);
    return std::string();
}
inline std::string ood_model_error(const fav_ood_model* m, int D_expected) {
    if (!m) return "model is NULL";
    if (m->struct_size != sizeof(fav_ood_model)) return fmt("struct_size=%u is not sizeof(fav_ood_model)=%zu", m->struct_size, sizeof(fav_ood_model));
    const std::string dims = ood_dims_error(m->D, m->k, m->R);
    if (!dims.empty()) return dims;
    if (D_expected >= 0 && m->D != D_expected) return fmt("D=%d is not the feature width %d of this arch", m->D, D_expected);
    if (!m->mu || !m->P || !m->M || !m->class_id) return "mu, P, M or class_id is NULL";
    if (std::isnan(m->threshold)) return "threshold is NaN";
    if (!ood_all_finite(m->mu, (size_t)m->D)) return "mu holds a non-finite value";
    if (!ood_all_finite(m->P, (size_t)m->k * m->D)) return "P holds a non-finite value";
    if (!ood_all_finite(m->M, (size_t)m->R * m->k)) return "M holds a non-finite value";
    for (int c = 0; c < m->R; ++c)
        if (m->class_id[c] < -1) return fmt("class_id[%d]=%d is below -1", c, m->class_id[c]);
    return std::string();
}

// frames a block: as many of 4, 2, 1 as the call has and as x and g of that many frames fit the LDS
inline int ood_frames_per_block(int n, int D, int k) {
    int fpb = n >= 4 ? 4 : (n >= 2 ? 2 : 1);
    while (fpb > 1 && (size_t)fpb * (size_t)(D + k) * 4 > (size_t)OOD_LDS_BYTES) fpb >>= 1;
    return fpb;
}

// fav_get_features: the tapped bf16 rows as fp32, eight values a thread (a row is a multiple of 16 values, both buffers come
// from hipMalloc or are checked for 16-byte alignment by the caller)
__global__ __launch_bounds__(256) void features_to_f32_kernel(const uint4* __restrict__ in, float4* __restrict__ out, long long groups) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < groups; e += (long long)gridDim.x * 256) {
        const uint4 v = in[e];
        out[2 * e] = make_float4(bf16_bits_to_f32(v.x & 0xFFFFu), bf16_bits_to_f32(v.x >> 16), bf16_bits_to_f32(v.y & 0xFFFFu), bf16_bits_to_f32(v.y >> 16));
        out[2 * e + 1] = make_float4(bf16_bits_to_f32(v.z & 0xFFFFu), bf16_bits_to_f32(v.z >> 16), bf16_bits_to_f32(v.w & 0xFFFFu), bf16_bits_to_f32(v.w >> 16));
    }
}

struct OodParams {
    const uint16_t* feat;        // [S][n][D] bf16
    const float* mu;             // [D]
    const float* Pt;             // [D][k]
    const float* Mt;             // [k][R]
    const int32_t* cls;          // [R]
    const int32_t* labels;       // [n] or NULL
    int32_t* rec;                // [n] fav_ood_record, 8-byte aligned
    int S, n, D, k, R;
    float inv_S, threshold;
};

// the FPB frames' values of one index, as they lie in LDS
template <int FPB> struct OodVec;
template <> struct OodVec<1> { float v[1]; };
template <> struct __align__(8) OodVec<2> { float v[2]; };
template <> struct __align__(16) OodVec<4> { float v[4]; };

template <int FPB>
__global__ __launch_bounds__(OOD_THREADS) void ood_score_kernel(const OodParams p) {
    using Vec = OodVec<FPB>;
    extern __shared__ __align__(16) float ood_lds[];
    float* const x = ood_lds;                       // [D][FPB]
    float* const g = ood_lds + (size_t)FPB * p.D;   // [k][FPB]
    __shared__ float w_best[OOD_WAVES][FPB], w_ld[OOD_WAVES][FPB];
    __shared__ int w_row[OOD_WAVES][FPB], w_lrow[OOD_WAVES][FPB];
    const int tid = threadIdx.x, D = p.D, k = p.k, R = p.R, n = p.n;
    const int i0 = blockIdx.x * FPB;

    // 1, 2: x = (sum_s feat[s]) * fp32(1 / S) - mu, eight neighbouring j of one frame a work item: one 16-byte load a sample
    // when the features are 16-byte aligned (a row is a multiple of 32 bytes), eight 2-byte loads when not.  Frames past n
    // are zero rows whose results nobody stores.
    const bool wide = ((uintptr_t)p.feat & 15) == 0;
    const int D8 = D >> 3;
    for (int e = tid; e < FPB * D8; e += OOD_THREADS) {
        const int f = e / D8, j0 = (e - f * D8) * 8, i = i0 + f;
        float sum[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) sum[q] = 0.f;
        if (i < n) {
            for (int s = 0; s < p.S; ++s) {
                const uint16_t* src = p.feat + ((size_t)s * n + i) * D + j0;
                uint32_t w[4];
                if (wide) {
                    const uint4 v = *(const uint4*)src;
                    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) w[q] = (uint32_t)src[2 * q] | ((uint32_t)src[2 * q + 1] << 16);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    sum[2 * q] = __fadd_rn(sum[2 * q], bf16_bits_to_f32(w[q] & 0xFFFFu));
                    sum[2 * q + 1] = __fadd_rn(sum[2 * q + 1], bf16_bits_to_f32(w[q] >> 16));
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) sum[q] = __fsub_rn(__fmul_rn(sum[q], p.inv_S), p.mu[j0 + q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) x[(j0 + q) * FPB + f] = sum[q];
    }
    __syncthreads();

    // 3: g[r] = sum_j P[r][j] * x[j], j ascending
    for (int r = tid; r < k; r += OOD_THREADS) {
        float acc[FPB];
#pragma unroll
        for (int f = 0; f < FPB; ++f) acc[f] = 0.f;
        const float* pt = p.Pt + r;
        for (int j0 = 0; j0 < D; j0 += 8) {         // D is a multiple of 16
            float pv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) pv[q] = pt[(size_t)(j0 + q) * k];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const Vec xv = *(const Vec*)(x + (size_t)(j0 + q) * FPB);
#pragma unroll
                for (int f = 0; f < FPB; ++f) acc[f] = __fadd_rn(acc[f], __fmul_rn(pv[q], xv.v[f]));
            }
        }
        Vec out;
#pragma unroll
        for (int f = 0; f < FPB; ++f) out.v[f] = acc[f];
        *(Vec*)(g + (size_t)r * FPB) = out;
    }
    __syncthreads();

    // 4 - 6: d[c] = sum_r (g[r] - M[c][r])^2, r ascending; a thread meets its rows c in ascending order
    float best[FPB], ld[FPB];
    int row[FPB], lrow[FPB], lab[FPB];
#pragma unroll
    for (int f = 0; f < FPB; ++f) {
        best[f] = INFINITY; row[f] = -1; ld[f] = 0.f; lrow[f] = INT_MAX;
        lab[f] = (p.labels && i0 + f < n) ? p.labels[i0 + f] : 0;
    }
    const bool has_labels = p.labels != nullptr;
    for (int c = tid; c < R; c += OOD_THREADS) {
        float acc[FPB];
#pragma unroll
        for (int f = 0; f < FPB; ++f) acc[f] = 0.f;
        const float* mt = p.Mt + c;
        int r0 = 0;
        for (; r0 + 8 <= k; r0 += 8) {
            float mv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) mv[q] = mt[(size_t)(r0 + q) * R];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const Vec gv = *(const Vec*)(g + (size_t)(r0 + q) * FPB);
#pragma unroll
                for (int f = 0; f < FPB; ++f) {
                    const float t = __fsub_rn(gv.v[f], mv[q]);
                    acc[f] = __fadd_rn(acc[f], __fmul_rn(t, t));
                }
            }
        }
        for (; r0 < k; ++r0) {
            const float mv = mt[(size_t)r0 * R];
            const Vec gv = *(const Vec*)(g + (size_t)r0 * FPB);
#pragma unroll
            for (int f = 0; f < FPB; ++f) {
                const float t = __fsub_rn(gv.v[f], mv);
                acc[f] = __fadd_rn(acc[f], __fmul_rn(t, t));
            }
        }
        const int cid = p.cls[c];
#pragma unroll
        for (int f = 0; f < FPB; ++f) {
            if (acc[f] < best[f]) { best[f] = acc[f]; row[f] = c; }
            if (has_labels && cid == lab[f] && c < lrow[f]) { lrow[f] = c; ld[f] = acc[f]; }
        }
    }
    // the wave's, then the block's: the smallest (d, row) - equal distances are finite here, or both rows are -1 - and the
    // lowest row of the label's class
#pragma unroll
    for (int f = 0; f < FPB; ++f) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best[f], off);
            const int orow = __shfl_xor(row[f], off);
            if (ob < best[f] || (ob == best[f] && orow < row[f])) { best[f] = ob; row[f] = orow; }
            const float old = __shfl_xor(ld[f], off);
            const int olrow = __shfl_xor(lrow[f], off);
            if (olrow < lrow[f]) { lrow[f] = olrow; ld[f] = old; }
        }
        if ((tid & 63) == 0) { w_best[tid >> 6][f] = best[f]; w_row[tid >> 6][f] = row[f]; w_ld[tid >> 6][f] = ld[f]; w_lrow[tid >> 6][f] = lrow[f]; }
    }
    __syncthreads();
    if (tid < FPB && i0 + tid < n) {
        float b = w_best[0][tid], l = w_ld[0][tid];
        int rw = w_row[0][tid], lr = w_lrow[0][tid];
        for (int w = 1; w < OOD_WAVES; ++w) {
            if (w_best[w][tid] < b || (w_best[w][tid] == b && w_row[w][tid] < rw)) { b = w_best[w][tid]; rw = w_row[w][tid]; }
            if (w_lrow[w][tid] < lr) { lr = w_lrow[w][tid]; l = w_ld[w][tid]; }
        }
        // 5 - 7: the record, as two 8-byte stores
        const int min_class = rw < 0 ? -1 : p.cls[rw];
        const float label_dist = lr == INT_MAX ? __int_as_float(0x7FC00000) : l;
        int2* out = (int2*)(p.rec + 4 * (size_t)(i0 + tid));
        out[0] = make_int2(__float_as_int(b), min_class);
        out[1] = make_int2(__float_as_int(label_dist), !(b <= p.threshold) ? 1 : 0);
    }
}

}  // namespace fav
