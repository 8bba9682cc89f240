// fav_rollout.hpp - attention rollout behind fav_set_attn_tap, fav_op_attn_mean, fav_op_attn_rollout, fav_rollout and
// fav_classify_rollout (include/fav.h; Abnar & Zuidema 2020).  The ViT counterpart of the class
// activation map: every layer's attention averaged over its heads, mixed half and half with the identity for the residual
// connection, the layers multiplied together; the class token's row of the product says how much each patch fed the decision.
// No backward pass.  The contract (fav.h, beside fav_set_attn_tap and fav_rollout_record) fixes every operation, so both
// kernels give the bits of a numpy restatement (tests/rollout_ref.py).
// Included by fav.hip after fav_kernels.hpp (fav_attn_softmax, the MFMA vector types), fav_route.hpp (fmt) and fav_mapbox.hpp
// (what the head's record shares with cam_kernel's: the box scan, the record store, the tap's budget check).
//
//   attn_mean_kernel       : the tap.  attention_kernel keeps its probabilities in registers and never writes them, so this
//                            kernel repeats its score product - the same MFMA chain with the same operands (K rows A, the
//                            lane's Q fragment B), without production's scheduling fences - calls fav_attn_softmax, which
//                            stands beside attention_kernel and holds its mask, max, exponential, partial sums and
//                            reciprocal (production keeps the statements in place: a call moved its schedule), and stops in
//                            front of the rounding to bf16.  A block takes one
//                            frame and up to four 16-query tiles, a wave a tile, and loops over the heads: the head's K lies
//                            in LDS (16 nkt rows of 128 B, the production swizzle), in two buffers - the next head's K and Q
//                            travel to registers under this head's MFMAs and exponentials and go to the other buffer behind
//                            them.  The lane holds 4 consecutive keys of one query per key tile (the S layout) and beside
//                            them the running head sum, 4 NKT registers more; one 16-byte store per lane and key tile.
//   attn_rollout_kernel    : the head.  A block a frame, a thread a column u of the running row r (in LDS, two buffers): the
//                            chain r'[u] = r'[u] + r[t] * A~[t][u] over t in index order, loads of eight t ahead of it.  The
//                            record is one lane's serial scans over the row: the kernel's own for the sum, the peak and the
//                            floor, then map_box_scan at the midpoint of a peak above the floor.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int ROLL_MAX_L = 64, ROLL_MAX_T = 256, ROLL_MAX_SIDE = 255, ROLL_THREADS = 256, ROLL_AHEAD = 8;
constexpr int ATTN_MEAN_WAVES = 4;                          // 16-query tiles a block takes, a wave each
constexpr size_t ATTN_TAP_DEFAULT_BUDGET = (size_t)2 << 30;  // fav_set_attn_tap's max_bytes = 0

inline int attn_ld(int T) { return 16 * ((T + 15) / 16); }

// ---- host: the one place the ranges live
inline std::string attn_mean_dims_error(int n, int T, int D, int heads) {
    if (n < 1) return "n must be at least 1";
    if (T < 2 || T > ROLL_MAX_T) return fmt("T=%d outside [2, %d]", T, ROLL_MAX_T);
    if (heads < 1 || heads > 64) return fmt("heads=%d outside [1, 64]", heads);
    if (D != 64 * heads) return fmt("D=%d is not 64 * heads=%d (the head width is 64)", D, heads);
    if ((long long)n * ((T + 15) / 16 + ATTN_MEAN_WAVES - 1) / ATTN_MEAN_WAVES > 0x7FFFFFFFll) return "n is too large for one grid";
    return std::string();
}
inline std::string rollout_dims_error(int L, int n, int gh, int gw, long long ld, int first_layer) {
    if (L < 1 || L > ROLL_MAX_L) return fmt("L=%d outside [1, %d]", L, ROLL_MAX_L);
    if (n < 1) return "n must be at least 1";
    if (gh < 1 || gw < 1 || gh > ROLL_MAX_SIDE || gw > ROLL_MAX_SIDE || gh * gw + 1 > ROLL_MAX_T)
        return fmt("gh=%d x gw=%d: a grid has sides of 1 to %d and at most %d cells (gh * gw + 1 tokens <= %d)", gh, gw, ROLL_MAX_SIDE,
                   ROLL_MAX_T - 1, ROLL_MAX_T);
    if (ld < gh * gw + 1 || ld % 4 != 0) return fmt("ld=%lld is not a multiple of 4 that is at least T=%d", ld, gh * gw + 1);
    if (first_layer < 0 || first_layer >= L) return fmt("first_layer=%d outside [0, L=%d)", first_layer, L);
    return std::string();
}

// what the attention tap of a ViT configuration holds
struct AttnTapDims { int L = 0, T = 0, ld = 0; size_t bytes = 0; };
inline AttnTapDims attn_tap_dims(int depth, int ntok, int max_batch) {
    AttnTapDims d;
    d.L = depth; d.T = ntok; d.ld = attn_ld(ntok);
    d.bytes = (size_t)depth * (size_t)max_batch * (size_t)ntok * d.ld * 4;
    return d;
}
// the configurations the tap refuses, from the config alone (nullptr: none)
inline const char* attn_tap_unsupported(int arch, int n_members, int math_mode) {
    if (n_members > 1) return "a deep ensemble is not supported (the ViT path has no ensemble mode)";
    if (arch != 2 && arch != 3) return "a ResNet arch has no attention; its localisation signal is the class activation map (fav_set_map_tap)";
    if (math_mode != 0) return "FAV_MATH_F32_EXACT is not supported: the tap restates the production score product only";
    return nullptr;
}

// ---- device: the tap
// qkv [n][T][3D] bf16 -> a [n][T][ldT] fp32, ldT = 16 * ceil(T / 16).  grid = n * ceil(nkt / nwaves) blocks of 64 * nwaves threads.
// NKT: key tiles the kernel is built for (T <= 16 NKT); FULL: T needs exactly NKT tiles, so every tile guard and the position
// of the masked tile are compile-time (the production shape), as in attention_kernel.  Neither the grid nor the block nor the
// instantiation changes a bit: a (query, key) element depends on its own Q and K rows and on the row's scores alone.
template <int NKT, bool FULL>
__global__ __launch_bounds__(64 * ATTN_MEAN_WAVES) void attn_mean_kernel(const uint16_t* __restrict__ qkv, float* __restrict__ a, int T, int D,
                                                                         int heads, float inv_heads) {
    extern __shared__ __attribute__((aligned(16))) unsigned char am_lds[];
    constexpr int CH = (NKT * 128 + 64 * ATTN_MEAN_WAVES - 1) / (64 * ATTN_MEAN_WAVES);   // 16-byte chunks of K a thread stages
    const int nkt = FULL ? NKT : (T + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x, nwaves = nthr >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int groups = (nkt + nwaves - 1) / nwaves;
    const long long f = blockIdx.x / groups;
    const int qt = (blockIdx.x % groups) * nwaves + wave;
    const bool active = qt < nkt;                  // wave-uniform
    const int q = qt * 16 + frow;                  // this lane's query (as MFMA column)
    const uint16_t* base = qkv + f * (long long)T * 3 * D;
    const int kbytes = nkt * 16 * 128;

    // the K chunks and the Q fragments of head h, into registers
    uint4 kv[CH], fqn[2];
    auto fetch = [&](int h) {
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const int i = tid + r * nthr, row = i >> 3, ch = i & 7;
            kv[r] = make_uint4(0u, 0u, 0u, 0u);
            if (row < T) kv[r] = *(const uint4*)(base + (long long)row * 3 * D + D + h * 64 + ch * 8);
        }
        fqn[0] = make_uint4(0u, 0u, 0u, 0u);
        fqn[1] = make_uint4(0u, 0u, 0u, 0u);
        if (active && q < T) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) fqn[kk] = *(const uint4*)(base + (long long)q * 3 * D + h * 64 + kk * 32 + fq * 8);
        }
    };
    // the staged chunks into K buffer b (zero beyond T)
    auto stage = [&](int b) {
        unsigned char* const Ks = am_lds + b * kbytes;
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const int i = tid + r * nthr, row = i >> 3, ch = i & 7;
            if (row < nkt * 16) *(uint4*)(Ks + row * 128 + ((ch ^ (row & 7)) << 4)) = kv[r];
        }
    };

    f32x4_t acc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) acc[kt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stage(0);
    __syncthreads();
    for (int h = 0; h < heads; ++h) {
        const unsigned char* const Ks = am_lds + (h & 1) * kbytes;
        const uint4 fqv[2] = {fqn[0], fqn[1]};
        if (h + 1 < heads) fetch(h + 1);           // travels while this head is computed
        if (active) {
            // ---- attention_kernel's score product, MODE 0
            f32x4_t sc[NKT];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                sc[kt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
                if (kt < nkt) {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const int row = kt * 16 + frow;
                        const uint4 fk = *(const uint4*)(Ks + row * 128 + (((kk * 4 + fq) ^ (row & 7)) << 4));
                        union { uint4 u; bf16x8_t v; } ua, ub;
                        ua.u = fk; ub.u = fqv[kk];
                        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, sc[kt], 0, 0, 0);
                    }
                }
            }
            // ---- attention_kernel's softmax: sc becomes the exponentials
            const float inv_sum = fav_attn_softmax<NKT, FULL>(sc, nkt, T, fq);
            // ---- the fp32 probability in front of production's rounding to bf16, added to the head sum: a product, then a sum
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
                if (kt < nkt) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[kt][j] = __fadd_rn(acc[kt][j], __fmul_rn(sc[kt][j], inv_sum));
                }
        }
        if (h + 1 < heads) stage((h + 1) & 1);     // the other buffer: its last readers passed the barrier of head h - 1
        __syncthreads();
    }
    if (active && q < T) {
        float* const row = a + (f * T + q) * (long long)(16 * nkt) + 4 * fq;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
            if (kt < nkt)
                *(float4*)(row + 16 * kt) = make_float4(__fmul_rn(acc[kt][0], inv_heads), __fmul_rn(acc[kt][1], inv_heads),
                                                        __fmul_rn(acc[kt][2], inv_heads), __fmul_rn(acc[kt][3], inv_heads));
    }
}

// ---- device: the head
struct RolloutParams {
    const float* a;              // layer l of frame i at a + l * layer_stride + i * T * ld; rows of ld fp32
    float* map;                  // [n][gh * gw]
    int32_t* rec;                // [n] fav_rollout_record, 8-byte aligned
    long long layer_stride;      // in floats
    int L, T, gw, ld, first_layer;
};

// A~[t][u] of the contract's step 1
__device__ __forceinline__ float rollout_mix(float a, int t, int u) { return __fadd_rn(__fmul_rn(0.5f, a), t == u ? 0.5f : 0.0f); }

__global__ __launch_bounds__(ROLL_THREADS) void attn_rollout_kernel(const RolloutParams p) {
    __shared__ float r_s[2][ROLL_MAX_T];
    const int u = threadIdx.x, T = p.T, i = blockIdx.x;
    const float* const Ai = p.a + (size_t)i * T * p.ld;
    // 2: the class token's row of the last layer
    if (u < T) r_s[0][u] = rollout_mix(Ai[(size_t)(p.L - 1) * p.layer_stride + u], 0, u);
    __syncthreads();
    int cur = 0;
    // 3: r' = r A~_l, a thread a column, t in index order
    for (int l = p.L - 2; l >= p.first_layer; --l) {
        const float* const Al = Ai + (size_t)l * p.layer_stride + u;
        if (u < T) {
            float acc = 0.f;
            for (int t0 = 0; t0 < T; t0 += ROLL_AHEAD) {
                float v[ROLL_AHEAD];
#pragma unroll
                for (int j = 0; j < ROLL_AHEAD; ++j) v[j] = t0 + j < T ? Al[(size_t)(t0 + j) * p.ld] : 0.f;
#pragma unroll
                for (int j = 0; j < ROLL_AHEAD; ++j)
                    if (t0 + j < T) acc = __fadd_rn(acc, __fmul_rn(r_s[cur][t0 + j], rollout_mix(v[j], t0 + j, u)));
            }
            r_s[cur ^ 1][u] = acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* const r = r_s[cur];
    const int HW = T - 1;
    // 4: the map
    if (u >= 1 && u < T) p.map[(size_t)i * HW + (u - 1)] = r[u];
    // 4 - 6: the record, by one lane: serial scans in index order
    if (u == 0) {
        float sum = 0.f, peak = -INFINITY, flo = INFINITY;
        int peak_cell = -1, n_above = 0, box = -1;
        for (int c = 0; c < HW; ++c) {
            const float v = r[1 + c];
            sum = __fadd_rn(sum, v);
            if (v > peak) { peak = v; peak_cell = c; }
            if (v < flo) flo = v;
        }
        if (peak > flo) n_above = map_box_scan(r + 1, HW, p.gw, __fadd_rn(flo, __fmul_rn(0.5f, __fsub_rn(peak, flo))), &box);
        map_record_store(p.rec + 8 * (size_t)i, p.L - p.first_layer, __float_as_int(r[0]), __float_as_int(peak), peak_cell,
                         __float_as_int(flo), __float_as_int(sum), n_above, box);
    }
}

}  // namespace fav
