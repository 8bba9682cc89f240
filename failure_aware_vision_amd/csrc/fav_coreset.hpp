// fav_coreset.hpp - greedy k-centre (farthest-point) selection behind fav_check_coreset, fav_coreset_workspace_bytes and
// fav_op_coreset_select (include/fav.h): which M rows of a pool of L2-normalised bf16 rows a
// patch bank or a k-NN bank keeps, so that the bank covers the feature space and does not sample its density (PatchCore; Roth
// et al. 2022).  The contract in fav.h fixes every operation, so order[] and radius[] are the bits of a numpy restatement
// (tests/coreset_ref.py):
//   c = order[t-1] taken;  sim = rows . rows[c] in 64 chains and six halving steps;  d = max(2 - 2 * sim, 0);
//   mind = min(mind, d);  (radius[t], order[t]) = the maximum of (mind, -row) over the rows not taken
// Included by fav.hip after fav_knn.hpp (KNN_MAX_D, KNN_MAX_N, knn_align).  One kernel, launched M + 1 times on the stream:
//
//   coreset_step_kernel : launch t = 0 .. M.  A grid of G blocks of 256 threads, G fixed for the call and at most 1024 (four
//                         blocks a CU); launch M is one block.  Every block first finds the centre of this step: start_row at
//                         t = 0, otherwise the maximum of the G partial (key, row) pairs launch t - 1 left (8 KB at most, read
//                         by every block: no second launch a step, no grid barrier, no atomics, no flag anybody spins on);
//                         block 0 also stores radius[t] and order[t].  The centre's row goes to LDS once a block.  Then the
//                         pool streams through: a wave a row, a lane 16 bytes a step at element 8 * lane + 512 * step, eight
//                         16-byte loads a lane issued ahead of their use (ROWS rows of STEPS steps), the first of them before
//                         the centre is known.  A lane's chain runs over its elements in ascending order, an xor butterfly
//                         folds the 64 chains.  mind is kept as uint32 keys - a non-negative float orders as its bits - and
//                         CORESET_TAKEN marks a taken row.  Launch 0 writes mind without reading it, every block writes its
//                         partial every launch: nothing an earlier call left in the workspace is ever read.  The partials
//                         are double-buffered by t & 1; stream order is the only synchronisation.
//                         A row is read once a launch: N * D * 2 bytes a step, which is all the traffic there is.  Below
//                         D = 512 only D / 8 lanes of a wave carry data.
#pragma once

namespace fav {

constexpr int CORESET_MAX_N = 1 << 24;
constexpr int CORESET_THREADS = 256, CORESET_WAVES = CORESET_THREADS / 64;
constexpr int CORESET_MAX_GRID = 1024;                       // blocks a launch, and slots of one partial buffer
constexpr int CORESET_AHEAD = 8;                             // 16-byte loads a lane has in flight: ROWS * STEPS
constexpr uint32_t CORESET_TAKEN = 0xFFFFFFFFu;              // the key of a taken row: above +inf, never a distance

// ---- host: the one place the ranges live (fav_check_coreset, fav_coreset_workspace_bytes, fav_op_coreset_select)
inline std::string coreset_error(int N, int D, int M, int start_row) {
    if (D < 64 || D > KNN_MAX_D || D % 64 != 0) return fmt("D=%d is not a multiple of 64 in [64, %d]", D, KNN_MAX_D);
    if (N < 1 || N > CORESET_MAX_N) return fmt("N=%d outside [1, %d]", N, CORESET_MAX_N);
    if (M < 1 || M > std::min(N, KNN_MAX_N)) return fmt("M=%d outside [1, min(N, %d)=%d]", M, KNN_MAX_N, std::min(N, KNN_MAX_N));
    if (start_row < 0 || start_row >= N) return fmt("start_row=%d outside [0, N=%d)", start_row, N);
    return std::string();
}

// rows a wave takes at a time, by the 512-element steps of one row: ROWS * STEPS = CORESET_AHEAD loads a lane
inline int coreset_rows_per_wave(int D) { return D <= 1024 ? 4 : D <= 2048 ? 2 : 1; }
inline int coreset_grid(int N, int D) {
    const int rpw = coreset_rows_per_wave(D);
    const long long groups = ((long long)N + rpw - 1) / rpw;
    return (int)std::min<long long>((groups + CORESET_WAVES - 1) / CORESET_WAVES, CORESET_MAX_GRID);
}

// The workspace: [ mind uint32 [N] | partials uint64 [2][CORESET_MAX_GRID] ], either part on a 256-byte boundary.
struct CoresetWs {
    size_t mind, part, bytes;
};
inline CoresetWs coreset_workspace(int N) {
    CoresetWs w;
    w.mind = 0;
    w.part = knn_align((size_t)N * 4);
    w.bytes = w.part + 2 * (size_t)CORESET_MAX_GRID * 8;
    return w;
}

// ---- device
struct CoresetParams {
    const uint16_t* rows;                // [N][D] bf16, 16-byte aligned
    uint32_t* mind;                      // [N] keys
    const unsigned long long* prev;      // [grid] what launch t - 1 wrote (not read at t = 0)
    unsigned long long* cur;             // [grid] what this launch writes (not at t = M)
    int32_t* order;                      // [M]
    float* radius;                       // [M + 1]
    int N, D, M, t, start_row, grid;     // grid: the blocks of a streaming launch, whatever this launch's own grid is
};

// (key, row) as one word whose unsigned order is the lexicographic order of (mind, -row); 0: a taken row, which loses to every
// other (a row is below 2^24, so no pair packs to 0)
__device__ __forceinline__ unsigned long long coreset_pack(uint32_t key, int row) {
    return key == CORESET_TAKEN ? 0ull : ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)row);
}
__device__ __forceinline__ unsigned long long coreset_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// acc + a[j] * b[j] over the eight bf16 of two 16-byte pieces, j ascending.  A product of two bf16 is exact in fp32, so the fma
// is the contract's multiply and add.
__device__ __forceinline__ float coreset_dot8(float acc, const uint4& a, const uint4& b) {
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc = __fmaf_rn(__uint_as_float(x[j] << 16), __uint_as_float(y[j] << 16), acc);
        acc = __fmaf_rn(__uint_as_float(x[j] & 0xFFFF0000u), __uint_as_float(y[j] & 0xFFFF0000u), acc);
    }
    return acc;
}

template <int ROWS, int STEPS>
__global__ __launch_bounds__(CORESET_THREADS) void coreset_step_kernel(const CoresetParams p) {
    static_assert(ROWS * STEPS == CORESET_AHEAD && STEPS * 512 <= KNN_MAX_D, "a wave's loads; launch_coreset picks STEPS * 512 >= D");
    __shared__ __attribute__((aligned(16))) uint16_t centre_s[KNN_MAX_D];
    __shared__ unsigned long long red_s[CORESET_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, D = p.D, t = p.t;
    const bool stream = t < p.M;                                   // launch M only closes the curve
    const long long groups = ((long long)N + ROWS - 1) / ROWS, stride = (long long)gridDim.x * CORESET_WAVES;
    long long g = (long long)blockIdx.x * CORESET_WAVES + wave;

    uint4 v[ROWS][STEPS];
    uint32_t old[ROWS];
    // the loads of group g: only elements below D and rows below N are read; the rest of v is zero and never used
    auto load = [&](long long grp) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const long long r = grp * ROWS + i;
            old[i] = 0;
            if (r < N && t > 0) old[i] = p.mind[r];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int el = lane * 8 + s * 512;
                v[i][s] = make_uint4(0u, 0u, 0u, 0u);
                if (r < N && el < D) v[i][s] = *(const uint4*)(p.rows + (size_t)r * D + el);
            }
        }
    };
    bool have = stream && g < groups;                              // the whole wave alike
    if (have) load(g);

    // 1: the centre of this step
    int c = p.start_row;
    if (t == 0) {
        if (blockIdx.x == 0 && tid == 0) { p.order[0] = c; p.radius[0] = INFINITY; }
    } else {
        unsigned long long best = 0;
        for (int i = tid; i < p.grid; i += CORESET_THREADS) best = coreset_max(best, p.prev[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = coreset_max(best, __shfl_xor(best, off));
        if (lane == 0) red_s[wave] = best;
        __syncthreads();
        best = red_s[0];
#pragma unroll
        for (int w = 1; w < CORESET_WAVES; ++w) best = coreset_max(best, red_s[w]);
        // none: every row is taken, which the ranges allow only at t == M == N
        c = best == 0 ? 0 : (int)(0xFFFFFFFFu - (uint32_t)best);
        if (blockIdx.x == 0 && tid == 0) {
            p.radius[t] = best == 0 ? 0.0f : __uint_as_float((uint32_t)(best >> 32));
            if (stream) p.order[t] = c;
        }
    }
    if (!stream) return;

    // 2: its row, once a block
    for (int el = tid * 8; el < D; el += CORESET_THREADS * 8) *(uint4*)(centre_s + el) = *(const uint4*)(p.rows + (size_t)c * D + el);
    __syncthreads();                                               // also: red_s has been read by every wave

    // 3: the pool
    unsigned long long mine = 0;
    while (have) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const long long r = g * ROWS + i;
            if (r < N) {                                           // the whole wave alike
                float acc = 0.0f;
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const int el = lane * 8 + s * 512;
                    if (el < D) acc = coreset_dot8(acc, v[i][s], *(const uint4*)(centre_s + el));
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off));   // every lane ends with s[0]
                const uint32_t key = __float_as_uint(fmaxf(__fsub_rn(2.0f, __fmul_rn(2.0f, acc)), 0.0f));
                uint32_t now = key;
                if (t > 0) now = old[i] == CORESET_TAKEN ? CORESET_TAKEN : (key < old[i] ? key : old[i]);
                if (r == c) now = CORESET_TAKEN;
                if (lane == 0 && (t == 0 || now != old[i])) p.mind[r] = now;
                mine = coreset_max(mine, coreset_pack(now, (int)r));
            }
        }
        g += stride;
        have = g < groups;
        if (have) load(g);
    }
    if (lane == 0) red_s[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long best = red_s[0];
#pragma unroll
        for (int w = 1; w < CORESET_WAVES; ++w) best = coreset_max(best, red_s[w]);
        p.cur[blockIdx.x] = best;
    }
}

// ---- host: the M + 1 launches of a call, on checked arguments.  Plain launches in stream order; each costs the host an
// enqueue, which a fit-time operation can afford.
inline void launch_coreset(const void* rows, int N, int D, int M, int start_row, void* ws, int32_t* order, float* radius, hipStream_t s) {
    const CoresetWs w = coreset_workspace(N);
    unsigned long long* const part = (unsigned long long*)((char*)ws + w.part);
    CoresetParams p;
    p.rows = (const uint16_t*)rows; p.mind = (uint32_t*)((char*)ws + w.mind); p.order = order; p.radius = radius;
    p.N = N; p.D = D; p.M = M; p.start_row = start_row; p.grid = coreset_grid(N, D);
    const int rpw = coreset_rows_per_wave(D);
    for (int t = 0; t <= M; ++t) {
        p.t = t;
        p.prev = part + (size_t)((t + 1) & 1) * CORESET_MAX_GRID;
        p.cur = part + (size_t)(t & 1) * CORESET_MAX_GRID;
        const dim3 grid((unsigned)(t < M ? p.grid : 1)), block(CORESET_THREADS);
        if (rpw == 4) hipLaunchKernelGGL((coreset_step_kernel<4, 2>), grid, block, 0, s, p);
        else if (rpw == 2) hipLaunchKernelGGL((coreset_step_kernel<2, 4>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((coreset_step_kernel<1, 8>), grid, block, 0, s, p);
    }
}

}  // namespace fav
