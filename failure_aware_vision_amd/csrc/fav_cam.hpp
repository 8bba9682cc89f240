// fav_cam.hpp - class activation maps behind fav_set_map_tap, fav_op_cam, fav_op_cam_heatmap, fav_cam and fav_classify_cam
// (include/fav.h; Zhou et al. 2016).  On a ResNet the logit of class c is the spatial mean of
// w_c . F(h, w) over the last feature map plus the bias, so M_c(h, w) = w_c . F(h, w) decomposes the logit over the cells of
// the map - no backward pass, and linear in the MC-Dropout samples.  The contract (fav.h, beside fav_cam_record) fixes every
// operation - fp32, one rounding per product and per sum, a fixed partition of the channels over 64 lanes, sums in index
// order - so the result is the bits of a numpy restatement (tests/cam_ref.py).
// Included by fav.hip after fav_plan.hpp (Plan), fav_route.hpp (fmt) and fav_mapbox.hpp (what the record shares with the
// rollout head's: the box scan, the record store, the tap's budget check).
//
//   cam_kernel<KT>      : one block of 1024 threads a frame, ONE launch and no global workspace, so the S x HW x C bf16 of a
//                         frame are read once for all K classes.  The K weight rows lie in LDS as bf16 (at most 64 KB), the K
//                         maps behind them as fp32 (at most 32 KB).  A wave owns a cell: lane l holds the channels
//                         512 m + 8 l .. + 7 of every 512-channel step - one 16-byte load a step, the loads of four steps
//                         issued ahead of their chain - and K running sums; six shuffle steps fold the 64 partials.  The head
//                         is bandwidth-bound (7.7 GFLOP against 1.5 GB at the headline shape), so the products and sums are
//                         plain v_mul_f32 / v_add_f32: the matrix pipe would buy nothing and would cost the fixed order.  The
//                         records are K serial scans in index order over a map in LDS, one lane each: the kernel's own
//                         for the sums, the peak and the floor, then map_box_scan at 20 % of a positive peak.
//   cam_heatmap_kernel  : a thread a pixel of the overlay: bilinear taps of the map, the record's floor and peak, one byte.
#pragma once

namespace fav {

using fav_route::fmt;

constexpr int CAM_MAX_K = 8, CAM_MAX_S = 4096, CAM_MAX_C = 4096, CAM_MAX_HW = 1024, CAM_MAX_SIDE = 256;
constexpr int CAM_THREADS = 1024, CAM_WAVES = CAM_THREADS / 64;
constexpr int CAM_STATIC_LDS = CAM_MAX_K * 4;                // cam_kernel's static LDS: the K checked class ids
constexpr int CAM_AHEAD = 4;                             // 16-byte loads a lane has in flight
constexpr size_t CAM_DEFAULT_BUDGET = (size_t)2 << 30;   // fav_set_map_tap's max_bytes = 0

// ---- host: the one place the head's ranges live (fav_op_cam, fav_cam, fav_classify_cam)
inline std::string cam_dims_error(int S, int n, int Hf, int Wf, int C, long long ldw, int n_classes, int K) {
    if (S < 1 || S > CAM_MAX_S) return fmt("S=%d outside [1, %d]", S, CAM_MAX_S);
    if (n < 1) return "n must be at least 1";
    if (Hf < 1 || Wf < 1 || Hf > CAM_MAX_SIDE || Wf > CAM_MAX_SIDE || Hf * Wf > CAM_MAX_HW)
        return fmt("Hf=%d x Wf=%d: a map has 1 to %d cells and sides of at most %d (the box packs a byte a coordinate)", Hf, Wf, CAM_MAX_HW, CAM_MAX_SIDE);
    if (C < 512 || C > CAM_MAX_C || C % 512 != 0) return fmt("C=%d is not a multiple of 512 in [512, %d]", C, CAM_MAX_C);
    if (ldw < C || ldw % 8 != 0) return fmt("ldw=%lld is not a multiple of 8 that is at least C=%d", ldw, C);
    if (n_classes < 1) return "n_classes must be at least 1";
    if (K < 1 || K > CAM_MAX_K) return fmt("K=%d outside [1, %d]", K, CAM_MAX_K);
    return std::string();
}
inline std::string cam_heatmap_dims_error(int m, int Hf, int Wf, int H, int W) {
    if (m < 1) return "m must be at least 1";
    if (Hf < 1 || Wf < 1 || Hf * Wf > CAM_MAX_HW) return fmt("Hf=%d x Wf=%d: a map has 1 to %d cells", Hf, Wf, CAM_MAX_HW);
    if (H < 1 || W < 1 || (long long)H * W > 0x7FFFFFFFll) return fmt("H=%d x W=%d: an overlay has 1 to 2^31 - 1 pixels", H, W);
    return std::string();
}

// ---- host: what the map tap of a planned schedule holds.  The maps are the input of the schedule's one OP_AVGPOOL; S: the
//      samples a frame has there (T_eff when the op runs once a sample, 1 when it lies in the prefix)
struct MapTapDims { int op = -1, S = 1, Hf = 0, Wf = 0, C = 0; size_t bytes = 0; };
inline MapTapDims map_tap_dims(const fav_plan::Plan& P, int max_batch) {
    MapTapDims d;
    for (const fav_plan::Phase& p : P.phases)
        for (int k = p.op_begin; k < p.op_end; ++k) {
            const fav_plan::Op& o = P.ops[k];
            if (o.kind != fav_plan::OP_AVGPOOL) continue;
            d.op = k; d.S = p.suffix ? P.T_eff : 1; d.Hf = o.H; d.Wf = o.W; d.C = o.C;
            d.bytes = (size_t)d.S * (size_t)max_batch * (size_t)o.H * o.W * o.C * 2;
        }
    return d;
}
// ---- host: what the stage tap of a planned schedule holds for residual stage 1 .. 4: the output of the op the planner marked
//      (Op::stage_out), copied behind its launch; S as above.  Stage 4 is the buffer the average pool reads, so its tap is the
//      map tap's own copy, in front of the pool (op: the pool; the same bytes under every dropout policy).  op < 0: no such stage
inline MapTapDims stage_tap_dims(const fav_plan::Plan& P, int max_batch, int stage) {
    if (stage == 4) return map_tap_dims(P, max_batch);
    MapTapDims d;
    for (const fav_plan::Phase& p : P.phases)
        for (int k = p.op_begin; k < p.op_end; ++k) {
            const fav_plan::Op& o = P.ops[k];
            if (stage < 1 || o.stage_out != stage) continue;
            d.op = k; d.S = p.suffix ? P.T_eff : 1; d.Hf = o.Ho; d.Wf = o.Wo; d.C = o.Co;
            d.bytes = (size_t)d.S * (size_t)max_batch * (size_t)o.Ho * o.Wo * o.Co * 2;
        }
    return d;
}
// the configurations the tap refuses, from the config alone (nullptr: none); the math mode makes no difference to it
inline const char* map_tap_unsupported(int arch, int n_members, int /*math_mode*/) {
    if (arch == 2 || arch == 3) return "a ViT arch has no pooled convolutional map";
    if (n_members > 1) return "the members of a deep ensemble have a map each; the map tap is not supported on it";
    return nullptr;
}

// ---- device
struct CamParams {
    const uint16_t* maps;        // [S][n][HW][C] bf16, 16-byte aligned
    const uint16_t* w;           // rows of ldw bf16, 16-byte aligned
    const float* bias;           // [n_classes]
    const int32_t* classes;      // [n][K]
    float* cam;                  // [n][K][HW]
    int32_t* rec;                // [n][K] fav_cam_record, 8-byte aligned
    int S, n, HW, Wf, C, K, n_classes;
    long long ldw;
    float inv_S, inv_HW;
};

__device__ __forceinline__ void cam_unpack8(const uint4 v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) { f[2 * q] = bf16_bits_to_f32(w[q] & 0xFFFFu); f[2 * q + 1] = bf16_bits_to_f32(w[q] >> 16); }
}

template <int KT>
__global__ __launch_bounds__(CAM_THREADS) void cam_kernel(const CamParams p) {
    extern __shared__ __align__(16) unsigned char cam_lds[];
    uint4* const wl = (uint4*)cam_lds;                                // [K][C / 8]: eight bf16 weights an entry
    float* const M = (float*)(cam_lds + (size_t)p.K * p.C * 2);       // [K][HW]
    __shared__ int cls_s[CAM_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, K = p.K, C = p.C, HW = p.HW, C8 = C >> 3;

    if (tid < K) {
        const int c = p.classes[(size_t)i * K + tid];
        cls_s[tid] = (c >= 0 && c < p.n_classes) ? c : -1;
    }
    __syncthreads();
    for (int e = tid; e < K * C8; e += CAM_THREADS) {
        const int k = e / C8, j = e - k * C8, c = cls_s[k];
        wl[e] = c >= 0 ? *(const uint4*)(p.w + (size_t)c * p.ldw + (size_t)j * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();

    // 1, 2: a wave a cell.  Step t = s * (C / 512) + m of the chain reads channels 512 m + 8 lane .. + 7 of sample s
    const int steps_per_sample = C >> 9, total = p.S * steps_per_sample;
    const size_t sample_stride = (size_t)p.n * HW * C;
    for (int hw = wave; hw < HW; hw += CAM_WAVES) {
        float acc[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] = 0.f;
        const uint16_t* cell = p.maps + ((size_t)i * HW + hw) * C + 8 * lane;
        int s = 0, m = 0;
        for (int t0 = 0; t0 < total; t0 += CAM_AHEAD) {
            uint4 v[CAM_AHEAD];
            int mq[CAM_AHEAD];
#pragma unroll
            for (int q = 0; q < CAM_AHEAD; ++q) {
                mq[q] = m;
                v[q] = make_uint4(0u, 0u, 0u, 0u);
                if (t0 + q < total) v[q] = *(const uint4*)(cell + (size_t)s * sample_stride + 512 * m);
                if (++m == steps_per_sample) { m = 0; ++s; }
            }
#pragma unroll
            for (int q = 0; q < CAM_AHEAD; ++q) {
                if (t0 + q < total) {
                    float x[8];
                    cam_unpack8(v[q], x);
#pragma unroll
                    for (int k = 0; k < KT; ++k) {
                        if (k < K) {
                            float wf[8];
                            cam_unpack8(wl[k * C8 + 64 * mq[q] + lane], wf);
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[k] = __fadd_rn(acc[k], __fmul_rn(wf[e], x[e]));
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            float a = acc[k];
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) a = __fadd_rn(a, __shfl_down(a, h));   // lane l < h: p[l] + p[l + h]
            if (lane == 0 && k < K) M[k * HW + hw] = __fmul_rn(a, p.inv_S);
        }
    }
    __syncthreads();

    // the maps: a slot whose class is out of range is all NaN
    const float qnan = __int_as_float(0x7FC00000);
    float* const cam = p.cam + (size_t)i * K * HW;
    for (int e = tid; e < K * HW; e += CAM_THREADS) cam[e] = cls_s[e / HW] >= 0 ? M[e] : qnan;

    // 3 - 6: the record of slot k, by lane 0 of wave k: serial scans in index order
    if (lane == 0 && wave < K) {
        const int k = wave, c = cls_s[k];
        const float* Mk = M + k * HW;
        float logit = qnan, peak = qnan, flo = qnan, pos = qnan;
        int peak_cell = -1, n_above = 0, box = -1;
        if (c >= 0) {
            float sum = 0.f;
            peak = -INFINITY; flo = INFINITY; pos = 0.f;
            for (int hw = 0; hw < HW; ++hw) {
                const float v = Mk[hw];
                sum = __fadd_rn(sum, v);
                if (v > peak) { peak = v; peak_cell = hw; }
                if (v < flo) flo = v;
                pos = __fadd_rn(pos, fmaxf(v, 0.f));
            }
            logit = __fadd_rn(__fmul_rn(sum, p.inv_HW), p.bias[c]);
            if (peak > 0.f) n_above = map_box_scan(Mk, HW, p.Wf, __fmul_rn(0.2f, peak), &box);
        }
        map_record_store(p.rec + 8 * ((size_t)i * K + k), c, __float_as_int(logit), __float_as_int(peak), peak_cell,
                         __float_as_int(flo), __float_as_int(pos), n_above, box);
    }
}

struct CamHeatParams {
    const float* cam;            // [m][Hf * Wf]
    const int32_t* rec;          // [m] fav_cam_record
    uint8_t* out;                // [m][H][W]
    int m, Hf, Wf, H, W;
    float scale_y, scale_x;      // (float)Hf / (float)H, (float)Wf / (float)W
};

// one axis of the bilinear tap: the source coordinate of output index o, its two cells and their weights
__device__ __forceinline__ void cam_tap(int o, float scale, int size, int* i0, int* i1, float* lo, float* hi) {
    const float src = fmaxf(__fsub_rn(__fmul_rn(__fadd_rn((float)o, 0.5f), scale), 0.5f), 0.f);
    *i0 = min((int)src, size - 1);
    *i1 = min(*i0 + 1, size - 1);
    *lo = __fsub_rn(src, (float)*i0);
    *hi = __fsub_rn(1.f, *lo);
}

__global__ __launch_bounds__(256) void cam_heatmap_kernel(const CamHeatParams p) {
    const long long per_map = (long long)p.H * p.W, total = per_map * p.m;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long j = idx / per_map;
        const int r = (int)(idx - j * per_map), y = r / p.W, x = r - y * p.W;
        const float peak = __int_as_float(p.rec[8 * j + 2]), flo = __int_as_float(p.rec[8 * j + 4]);
        uint8_t g = 0;
        if (peak > flo) {
            int y0, y1, x0, x1;
            float ly, hy, lx, hx;
            cam_tap(y, p.scale_y, p.Hf, &y0, &y1, &ly, &hy);
            cam_tap(x, p.scale_x, p.Wf, &x0, &x1, &lx, &hx);
            const float* M = p.cam + j * (long long)(p.Hf * p.Wf);
            const float top = __fadd_rn(__fmul_rn(hx, M[y0 * p.Wf + x0]), __fmul_rn(lx, M[y0 * p.Wf + x1]));
            const float bot = __fadd_rn(__fmul_rn(hx, M[y1 * p.Wf + x0]), __fmul_rn(lx, M[y1 * p.Wf + x1]));
            const float v = __fadd_rn(__fmul_rn(hy, top), __fmul_rn(ly, bot));
            const float t = __fdiv_rn(__fsub_rn(v, flo), __fsub_rn(peak, flo));
            g = (uint8_t)rintf(__fmul_rn(fminf(fmaxf(t, 0.f), 1.f), 255.f));
        }
        p.out[idx] = g;
    }
}

}  // namespace fav
