// fav.hip — executor and C ABI (include/fav.h) of the MI355X-native
// failure-aware classification path.
//
// Host side of the hot path: a static schedule of kernel launches on ONE HIP
// stream (handle is single-caller, like the reference's per-connection scorer,
// platform/backend/main.py:110-118; an ensemble's members and a ViT batch's parts
// fork from it and join it), a workspace arena allocated once, and
// Infinity-Cache-sized passes: frames go through the high-resolution stages in
// chunks small enough that producer->consumer activations stay in the 256 MiB
// L3, then through the low-resolution stages in larger chunks that fill the
// 256 CUs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fav.h"
#include "fav_kernels.hpp"
#include "fav_corrupt_c.hpp"
#include "fav_plan.hpp"
#include "fav_route.hpp"
#include "fav_views.hpp"
#include "fav_ood.hpp"
#include "fav_knn.hpp"
#include "fav_drift.hpp"
#include "fav_mapbox.hpp"
#include "fav_cam.hpp"
#include "fav_rollout.hpp"
#include "fav_curve.hpp"
#include "fav_rise.hpp"
#include "fav_patch.hpp"
#include "fav_coreset.hpp"
#include "fav_ae.hpp"

using namespace fav_plan;    // the schedule: Plan, Op, Phase, the planner and the rules it shares with the launchers
using namespace fav_route;   // the selector: which kernel a launch takes, on what grid (Route)

namespace {

thread_local std::string g_create_error;

// ---- route report (fav_op_last_route, fav.h): which kernel instantiation the calling thread's last launch took.  A launcher
//      stores the Route it launches from (fav_route.hpp); text is formatted only when somebody asks.
thread_local Route g_route;

// the launchers with one kernel and no selector (entry reduce, fused stem)
inline void route_set(int kind, int a0 = 0, int a1 = 0) {
    Route r;
    r.kind = kind; r.a[0] = a0; r.a[1] = a1;
    g_route = r;
}
inline void route_clear() { g_route.kind = ROUTE_NONE; g_route.fresh = false; }
// at the end of a fav_op_*: a refusal, or a launch through a launcher that records nothing, leaves no route behind
inline void route_close(bool ok) {
    if (!ok || !g_route.fresh) g_route.kind = ROUTE_NONE;
    g_route.fresh = false;
}

// inside a fork/join region: remember the first failure but keep going, so that every forked stream is joined
#define HIP_KEEP(h, st, expr)                                                                    \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess && (st) == FAV_OK) {                                                \
            (h)->err = fmt("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            (st) = FAV_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (h)->err = fmt("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FAV_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

inline bool is_vit_arch(int arch) { return arch == 2 || arch == 3; }

struct LayerWeights {  // the device side of one plan layer
    std::vector<uint16_t*> w_m;     // per ensemble member: w_slab + member * w_stride (one allocation, so that a grouped
    std::vector<float*> b_m;        // launch reaches member g's weights at a constant stride); a single model is member 0
    void *w_slab = nullptr, *b_slab = nullptr;
    size_t w_stride = 0, b_stride = 0;
};

// What a grouped launch adds to a launch: every op of the schedule is ONE launch over all members - block row blockIdx.y is
// member y, whose tensors lie at a constant byte stride behind member 0's (the workspaces and the weights are slabs).
// run_chunks builds it per op and hands it to the launcher; default-constructed: one member, no strides.
struct Group { int n = 1; long long x = 0, w = 0, b = 0, res = 0, y = 0, wb = 0, bb = 0, wa = 0, ba = 0, y2 = 0; };

// Where run_chunks launches: a stream, a workspace, a member's weights.  Every handle has at least one lane: a single model
// is lane 0 on the caller's stream; an ensemble has one lane per member on the member's own stream, and a grouped call runs
// lane 0 on the caller's stream with groups = n_members.  The buffers are views: the handle owns (and frees) the slabs.
struct Lane {
    hipStream_t stream = nullptr;   // the member's own stream (an ensemble); a call on the caller's stream fills in its copy
    hipEvent_t done = nullptr;      // with `stream`: the member's join
    void* act[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    void* a1 = nullptr;
    void* phase_out[kMaxPhases] = {nullptr, nullptr, nullptr, nullptr};   // all but the last phase's, which writes the logits
    int member = 0;                 // whose weights, and whose slot of the logits
    int groups = 1;                 // > 1: every op one launch over this many members, from this lane's at a constant stride
};

// The frames of one call
struct Frames { const void* images; int layout; int n; long long first_index; };

}  // namespace

struct fav_handle {
    fav_config cfg;
    std::string err;
    Plan plan;                         // what runs: layer shapes, ops, phases (fav_plan.hpp)
    std::vector<LayerWeights> weights; // one entry per plan layer
    bool weights_loaded = false;
    std::vector<char> member_loaded;   // deep ensemble (BASELINE configs[3]): one checkpoint per member
    int n_members = 1;
    // workspace: the slabs (n_members equal parts each for an ensemble, so that a grouped launch finds member g's tensors at a
    // constant stride); the lanes hold views into them
    void* act[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t act_bytes = 0;
    hipEvent_t ev_fork = nullptr;   // ViT: the fork of a split batch
    void* a1 = nullptr;
    size_t a1_bytes = 0;
    // One lane per member (a single model: lane 0, no stream of its own).  Deep ensemble (BASELINE configs[3]): the members are
    // independent networks over the same frames, so each runs on its own stream with its own rotating buffers and the head
    // waits for all of them - at the per-GPU share of 32 frames a single member leaves most CUs idle in layers 3-4 - unless
    // the call is grouped (will_group).  (The members one after another on the caller's stream: 4 290 against 7 580 frames/s
    // at 32 frames per call; the code is gone, its record is tools/experiments/ensemble_serial_members.diff.)
    std::vector<Lane> lanes;
    hipEvent_t ev_members = nullptr;
    std::vector<hipStream_t> vit_streams;   // ViT: parts of the batch side by side
    std::vector<hipEvent_t> vit_done;
    // chained stream-K GEMM (gemm_streamk_kernel): one workspace per stream the encoder may run on (slot 0: the caller's)
    struct SkWs { float* ws = nullptr; uint32_t* flags = nullptr; uint32_t* err = nullptr; uint32_t epoch = 0; int grid_cap = 0; };
    SkWs sk[5];
    int sk_slot = 0;                        // the slot run_vit's launches use
    std::vector<void*> phase_out;   // output slab of each phase but the last (whose output is the logits)
    float* logits = nullptr;        // [T][max_batch][cpad]
    int last_T = 0, last_n = 0;
    void* host_stage = nullptr;     // for fav_classify_host
    hipStream_t host_stream = nullptr;
    // Every call that touches the handle's buffers (act[], a1, phase outputs, logits) records ev_last on its stream when it has
    // queued its work, and the next call makes ITS stream wait for that event first: two calls on different streams (a torch
    // stream and host_stream, or two torch streams) are then ordered on the device instead of racing on the activations.
    hipEvent_t ev_last = nullptr;
    bool ev_last_set = false;
    // Test-time augmentation (fav_set_views): the views in force (n_views = 0: off) and the buffer a call's frames are expanded
    // into, [n_views][n] frames of the call's layout; allocated by the first call that needs it, for max_batch frames
    fav_view views[FAV_MAX_VIEWS];
    int n_views = 0;
    void* view_buf = nullptr;
    size_t view_buf_bytes = 0;
    // Feature tap (fav_set_feature_tap): while on, every pass copies the rows its fc launch reads into feat_buf, bf16
    // [T_head][max_batch][feat_D] at most, indexed [sample][frame] like the logits; allocated by the setter.  feat_T / feat_n:
    // the samples and frames of the last call that filled it (0: none yet).  tap_user: fav_set_feature_tap(1) is in force.
    // tap is derived: tap_user || ood_on || knn_on || drift_on, as tap_sync last brought it in line
    bool tap = false, tap_user = false;
    void* feat_buf = nullptr;
    int feat_D = 0, feat_T = 0, feat_n = 0;
    // OOD model (fav_set_ood): the device copy, P and M transposed (fav_ood.hpp); ood_on: one is set
    struct OodDev { float *mu = nullptr, *Pt = nullptr, *Mt = nullptr; int32_t* cls = nullptr; int D = 0, k = 0, R = 0; float threshold = 0.f; };
    OodDev ood;
    bool ood_on = false;
    // k-NN bank (fav_set_knn): the device copy, padded with zero rows to Npad, and the head's workspace for max_batch frames
    // (fav_knn.hpp knn_workspace, its zero bias written once by the setter); knn_on: one is set
    struct KnnDev { void *bank = nullptr, *ws = nullptr; int32_t* cls = nullptr; int D = 0, N = 0, k = 0; float threshold = 0.f; };
    KnnDev knn;
    bool knn_on = false;
    // patch bank (fav_set_patch_bank): the device copy, padded with zero rows to Npad, and the head's workspace for max_batch *
    // Hf * Wf cells (fav_patch.hpp patch_workspace, its zero bias written once by the setter); Hf, Wf: the planner's map, which
    // the map tap holds when it is on.  patch_on: one is set.  It reads the map tap and never turns it on or off
    // stage, radius: the site (fav_set_patch_bank_at; stage 0: none - the map tap and the k-NN head's query kernel, radius -1)
    struct PatchDev { void *bank = nullptr, *ws = nullptr; int D = 0, N = 0, chunk_rows = 0, Hf = 0, Wf = 0; float threshold = 0.f;
                      int stage = 0, radius = -1; };
    PatchDev patch;
    bool patch_on = false;
    // drift reference (fav_set_drift): the workspace for max_batch frames (fav_drift.hpp drift_workspace, cached_ref), its
    // pool holding the reference and U the reference's block of distances, both written once by the setter; drift_on: one is set
    struct DriftDev { void* ws = nullptr; int D = 0, R = 0, n_perm = 0; uint64_t seed = 0; float alpha = 0.f; };
    DriftDev drift;
    bool drift_on = false;
    // The two localisation taps, each the caller's own (the feature tap above is derived from its readers), share one record:
    // on, the buffer (allocated by the setter for max_batch frames, freed when the tap goes off), and what the last call that
    // filled it left - S x n: its samples and frame rows (n = 0: none yet; S stays 0 where a frame has no samples), views: the
    // views it ran under.  The steps on it: tap_off .. classify_map_head below.
    struct LocTap { bool on = false; void* buf = nullptr; int S = 0, n = 0, views = 0; };
    // Map tap (fav_set_map_tap): while on, every pass copies the frames its average pool reads into map_tap.buf, bf16
    // [map.S][max_batch][Hf * Wf][C] at most (map: fav_cam.hpp map_tap_dims of the plan), indexed [sample][frame] like the logits
    LocTap map_tap;
    fav::MapTapDims map;
    // Stage tap (fav_set_stage_tap): while on, every pass copies the frames op stage.op of the plan has written (stage 4: the
    // frames the pool reads, as the map tap) into stage_tap.buf, laid out like the map tap's; stage_no: the stage in force (0: off)
    LocTap stage_tap;
    fav::MapTapDims stage;
    int stage_no = 0;
    // Attention tap (fav_set_attn_tap; ViT only): while on, every encoder layer of every run_vit part launches attn_mean_kernel
    // (fav_rollout.hpp) in front of its attention launch; attn_tap.buf holds fp32 [attn.L][n][attn.T][attn.ld] for the n frame
    // rows of the call (at most max_batch), a part at its frame offset
    LocTap attn_tap;
    fav::AttnTapDims attn;
    // The two perturbation heads (fav_set_curve, fav_set_rise) share one record: ONE buffer the setter allocates for max_batch
    // frames, with its parts - frames (the occluded or masked frames of one pass, sized for fp32), prob (the planes
    // [passes][max_batch]; passes = steps + 1 or n_masks + 1), lab0 and conf0 (the unperturbed pass's label and confidence),
    // and the curve head's own rank [max_batch][1024] and lab (planes like prob), both null for RISE.  Each stands beside
    // the descriptor in force and its flag (one is set).  The steps on it: perturb_clear .. classify_perturb_head below.
    struct PerturbDev { void* buf = nullptr; void* frames = nullptr; float* prob = nullptr; int32_t* lab0 = nullptr; float* conf0 = nullptr;
                        int32_t* rank = nullptr; int32_t* lab = nullptr; int passes = 0; };
    fav_curve curve_desc{};
    PerturbDev curve;
    bool curve_on = false;
    fav_rise rise_desc{};
    PerturbDev rise;
    bool rise_on = false;
    // ViT path (arch 2, 3): layers in blob order (kh == 0: a pair of fp32 vectors kept in w_m / b_m), fixed buffers
    bool vit = false;
    void *v_patches = nullptr, *v_emb = nullptr, *v_x = nullptr, *v_y = nullptr, *v_qkv = nullptr, *v_hid = nullptr, *v_cls = nullptr;
    // profiling
    bool profiling = false;
    struct Ev { hipEvent_t a, b; int cls; int op; };
    std::vector<fav_op_profile> op_prof;   // one row per op of the static schedule
    int cur_op = -1;
    std::vector<Ev> ev_pool;
    size_t ev_used = 0;
    fav_profile prof{};
};

namespace {

using namespace fav;

// the experiment knobs (FAV_KNOB, fav_plan.hpp) that are text
#ifdef FAV_EXPERIMENTS
const char* fav_knob_str(const char* name) { return getenv(name); }
#else
const char* fav_knob_str(const char*) { return nullptr; }
#endif

// ------------------------------------------------------------------ launchers
struct Prof {
    fav_handle* h;
    hipStream_t s;
    int idx = -1;
    Prof(fav_handle* h_, hipStream_t s_, int cls, double flops, double bytes) : h(h_), s(s_) {
        if (!h || !h->profiling) return;
        if (h->ev_used == h->ev_pool.size()) {
            fav_handle::Ev e;
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
            h->ev_pool.push_back(e);
        }
        idx = (int)h->ev_used++;
        h->ev_pool[idx].cls = cls;
        h->ev_pool[idx].op = h->cur_op;
        if (h->cur_op >= 0 && h->cur_op < (int)h->op_prof.size()) {
            h->op_prof[h->cur_op].flops += flops;
            h->op_prof[h->cur_op].bytes += bytes;
            h->op_prof[h->cur_op].launches += 1;
        }
        h->prof.flops[cls] += flops;
        h->prof.bytes[cls] += bytes;
        h->prof.launches[cls] += 1;
        (void)hipEventRecord(h->ev_pool[idx].a, s);
    }
    ~Prof() {
        if (idx >= 0) (void)hipEventRecord(h->ev_pool[idx].b, s);
    }
};

// Per-device "done once" flags: a process may hold handles on several devices (fav_config.device), and a
// function attribute such as the dynamic-LDS limit is a property of (kernel, device).
struct DeviceFlags {
    std::atomic<unsigned long long> bits[2] = {};   // up to 128 device ordinals
    static int current() { int d = 0; (void)hipGetDevice(&d); return (d < 0 || d >= 128) ? 0 : d; }
    bool test_current() const { const int d = current(); return (bits[d >> 6].load(std::memory_order_acquire) >> (d & 63)) & 1ull; }
    void set_current() { const int d = current(); bits[d >> 6].fetch_or(1ull << (d & 63), std::memory_order_release); }
};

DropParams make_drop(const fav_dropout_desc* d) {
    DropParams p;
    if (!d || d->site < 0) {
        p.site = -1; p.thr = 0; p.scale = 1.f; p.seed_lo = p.seed_hi = 0; p.v0 = 0; p.n_img = 1; p.first_index = 0;
        p.div_img = fastdiv_make(1);
        return p;
    }
    p.site = d->site;
    p.thr = d->threshold;
    p.scale = d->scale;
    p.seed_lo = (uint32_t)(d->seed & 0xFFFFFFFFull);
    p.seed_hi = (uint32_t)(d->seed >> 32);
    p.v0 = d->v0;
    p.n_img = d->n_img > 0 ? d->n_img : 1;
    p.first_index = d->first_image_index;
    p.div_img = fastdiv_make((uint32_t)p.n_img);
    return p;
}

// ---- kernel tables: one per kernel family, from a Route's kind and template arguments to the instantiation (all of a family
//      share one signature).  They name every instantiation the build contains, those only an experiment knob reaches too.
template <class Fn> struct KernelEntry { int kind; int a[8]; Fn fn; mutable DeviceFlags lds_set; };   // lds_set: see find_kernel
using ConvKernel = void (*)(const ConvParams);
using HaloKernel = void (*)(const ConvParams, int);
using TailKernel = void (*)(const TailParams, int);
using AttnKernel = void (*)(const uint16_t*, uint16_t*, int, int, int);

template <int BM, int BN, int BK, int NS, int MODE, int EPI, int PP = 0, bool GELU = false>
KernelEntry<ConvKernel> igemm() { return {ROUTE_CONV_IGEMM, {BM, BN, BK, NS, MODE, EPI, PP, GELU}, conv_igemm_kernel<BM, BN, BK, NS, MODE, 2, 0, EPI, PP, GELU>}; }
template <int CIN, int BN, int BM, int NS, int SUB, int OCC, int MODE>
KernelEntry<HaloKernel> halo() { return {ROUTE_CONV_HALO, {CIN, BN, BM, NS, MODE}, conv3x3_halo_kernel<CIN, BN, BM, NS, SUB, OCC, MODE>}; }
template <int CMID, int NRED, bool H3, int NS, int NW, bool WC2, int RP = 32, bool RESE = false>
KernelEntry<TailKernel> tail() { return {ROUTE_TAIL, {CMID, NRED, H3, NW, WC2, RP, RESE}, bottleneck_tail_kernel<CMID, NRED, H3, NS, NW, WC2, RP, 0, true, true, RESE>}; }
template <int MODE, int NKT, bool FULL = false>
KernelEntry<AttnKernel> attn() { return {ROUTE_ATTENTION, {MODE, NKT, FULL}, attention_kernel<MODE, NKT, FULL>}; }

// 128-row tiles: BN 64 | 128, 32-deep steps in a three-stage ring or 64-deep in two, both math modes, both epilogues, with and
// without the GELU; 256 x 256 x 64: the ping-pong loop in the production mode, the plain one in both (FAV_CONV_PP, FAV_CONV_EPI)
const KernelEntry<ConvKernel> kConvKernels[] = {
    igemm<128, 64, 32, 3, 0, 0>(), igemm<128, 64, 32, 3, 0, 1>(), igemm<128, 64, 32, 3, 0, 0, 0, true>(), igemm<128, 64, 32, 3, 0, 1, 0, true>(),
    igemm<128, 64, 32, 3, 1, 0>(), igemm<128, 64, 32, 3, 1, 1>(), igemm<128, 64, 32, 3, 1, 0, 0, true>(), igemm<128, 64, 32, 3, 1, 1, 0, true>(),
    igemm<128, 64, 64, 2, 0, 0>(), igemm<128, 64, 64, 2, 0, 1>(), igemm<128, 64, 64, 2, 0, 0, 0, true>(), igemm<128, 64, 64, 2, 0, 1, 0, true>(),
    igemm<128, 64, 64, 2, 1, 0>(), igemm<128, 64, 64, 2, 1, 1>(), igemm<128, 64, 64, 2, 1, 0, 0, true>(), igemm<128, 64, 64, 2, 1, 1, 0, true>(),
    igemm<128, 128, 32, 3, 0, 0>(), igemm<128, 128, 32, 3, 0, 1>(), igemm<128, 128, 32, 3, 0, 0, 0, true>(), igemm<128, 128, 32, 3, 0, 1, 0, true>(),
    igemm<128, 128, 32, 3, 1, 0>(), igemm<128, 128, 32, 3, 1, 1>(), igemm<128, 128, 32, 3, 1, 0, 0, true>(), igemm<128, 128, 32, 3, 1, 1, 0, true>(),
    igemm<128, 128, 64, 2, 0, 0>(), igemm<128, 128, 64, 2, 0, 1>(), igemm<128, 128, 64, 2, 0, 0, 0, true>(), igemm<128, 128, 64, 2, 0, 1, 0, true>(),
    igemm<128, 128, 64, 2, 1, 0>(), igemm<128, 128, 64, 2, 1, 1>(), igemm<128, 128, 64, 2, 1, 0, 0, true>(), igemm<128, 128, 64, 2, 1, 1, 0, true>(),
    igemm<256, 256, 64, 2, 0, 1, 1>(), igemm<256, 256, 64, 2, 0, 1, 1, true>(),
    igemm<256, 256, 64, 2, 0, 0>(), igemm<256, 256, 64, 2, 0, 1>(), igemm<256, 256, 64, 2, 0, 0, 0, true>(), igemm<256, 256, 64, 2, 0, 1, 0, true>(),
    igemm<256, 256, 64, 2, 1, 0>(), igemm<256, 256, 64, 2, 1, 1>(), igemm<256, 256, 64, 2, 1, 0, 0, true>(), igemm<256, 256, 64, 2, 1, 1, 0, true>(),
};
// 256-pixel tiles; the 128-pixel ones are FAV_HALO_CFG=0's
const KernelEntry<HaloKernel> kHaloKernels[] = {
    halo<64, 64, 256, 3, 1, 4, 0>(), halo<64, 64, 256, 3, 1, 4, 1>(), halo<128, 128, 256, 2, 2, 2, 0>(), halo<128, 128, 256, 2, 2, 2, 1>(),
    halo<64, 64, 128, 2, 1, 3, 0>(), halo<64, 64, 128, 2, 1, 3, 1>(), halo<128, 128, 128, 2, 1, 2, 0>(), halo<128, 128, 128, 2, 1, 2, 1>(),
};
// 64 mid channels: 4 waves, a three-stage ring; 128: 8 waves; each with two Wc buffers or one; layers 3 and 4; the res_entry
// pair; and the projections, which are the tail kernel without conv_b, residual and ReLU at a fixed Cout
const KernelEntry<TailKernel> kTailKernels[] = {
    tail<64, 0, true, 3, 4, true>(), tail<64, 0, true, 3, 4, false>(), tail<64, 64, true, 3, 4, true>(), tail<64, 64, true, 3, 4, false>(),
    tail<64, 128, true, 3, 4, true>(), tail<64, 128, true, 3, 4, false>(),
    tail<64, 0, false, 3, 4, true>(), tail<64, 0, false, 3, 4, false>(), tail<64, 64, false, 3, 4, true>(), tail<64, 64, false, 3, 4, false>(),
    tail<64, 128, false, 3, 4, true>(), tail<64, 128, false, 3, 4, false>(),
    tail<128, 0, true, 2, 8, true>(), tail<128, 0, true, 2, 8, false>(), tail<128, 128, true, 2, 8, true>(), tail<128, 128, true, 2, 8, false>(),
    tail<128, 0, false, 2, 8, true>(), tail<128, 0, false, 2, 8, false>(), tail<128, 128, false, 2, 8, true>(), tail<128, 128, false, 2, 8, false>(),
    tail<512, 0, false, 2, 8, true>(), tail<256, 0, true, 2, 8, true>(), tail<256, 0, false, 2, 4, true>(), tail<256, 0, false, 2, 4, false>(),
    tail<256, 256, false, 2, 8, true, 16>(), tail<256, 256, false, 2, 8, false, 16>(),
    tail<64, 64, true, 3, 4, true, 32, true>(), tail<64, 64, true, 3, 4, false, 32, true>(),
    {ROUTE_PROJ, {256, 512, 4}, bottleneck_tail_kernel<256, 0, false, 2, 4, true, 32, 512, false, false>},
    {ROUTE_PROJ, {512, 1024, 8}, bottleneck_tail_kernel<512, 0, false, 2, 8, true, 32, 1024, false, false>},
};
const KernelEntry<AttnKernel> kAttnKernels[] = {attn<0, 13, true>(), attn<0, 13>(), attn<0, 16>(), attn<1, 13>(), attn<1, 16>()};

// The table's kernel for a Route, nullptr if it has none.  A kernel with dynamic LDS has its limit raised first, once per
// (entry, device): hipFuncSetAttribute applies to the CURRENT device only; *lds_ok says whether that worked.
template <class Fn, size_t N>
Fn find_kernel(const KernelEntry<Fn> (&table)[N], const Route& r, bool* lds_ok) {
    *lds_ok = true;
    for (const KernelEntry<Fn>& e : table) {
        if (e.kind != r.kind || memcmp(e.a, r.a, sizeof r.a) != 0) continue;
        if (r.lds > 0 && !e.lds_set.test_current()) {
            *lds_ok = hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
            if (*lds_ok) e.lds_set.set_current();
        }
        return e.fn;
    }
    return nullptr;
}

// the tail kernel's parameters that do not depend on what feeds it: geometry, the LDS plan, fast divisions
TailParams tail_params(const Route& r) {
    TailParams p;
    memset(&p, 0, sizeof p);
    p.H = r.Ho; p.W = r.Wo; p.HW = r.Ho * r.Wo; p.M = r.M;
    p.in_W = p.W; p.in_HW = p.HW; p.in_stride = 1;
    const TailGeom& g = r.geom;
    p.rega_bytes = g.rega_bytes;
    p.bias_b_off = g.bias_b_off; p.bias_ca_off = g.bias_ca_off; p.wa_off0 = g.wa_off0; p.wa_off1 = g.wa_off1; p.zero_off = g.zero_off;
    p.div_hw = fastdiv_make((uint32_t)p.HW);
    p.div_w = fastdiv_make((uint32_t)p.W);
    p.rs_T = r.rs_T; p.rs_tps = r.rs_tps;
    return p;
}

// the projection shortcut (route_proj): the tail kernel as a strided 1x1
const char* launch_proj(fav_handle* h, const fav_conv_desc& d, const Route& r, const Group& G, hipStream_t s) {
    TailParams p = tail_params(r);
    p.t1 = (const uint16_t*)d.x; p.wc = (const uint16_t*)d.w; p.bias_c = d.bias; p.y = (uint16_t*)d.y;
    p.in_W = d.W; p.in_HW = d.H * d.W; p.in_stride = d.stride;
    p.drop = make_drop(nullptr);
    p.g_t1 = G.x; p.g_wc = G.w; p.g_bc = G.b; p.g_y = G.y;
    bool lds_ok;
    const TailKernel kern = find_kernel(kTailKernels, r, &lds_ok);
    if (!kern || !lds_ok) return kern ? "conv: cannot reserve LDS for the projection kernel" : "conv: no kernel for this route";
    const double flops = 2.0 * (double)r.M * d.Cin * d.Cout * G.n;
    const double bytes = 2.0 * ((double)r.M * (d.Cin + d.Cout) + (double)d.Cin * d.Cout) * G.n;
    Prof pr(h, s, FAV_K_CONV, flops, bytes);
    g_route = r;
    hipLaunchKernelGGL(kern, dim3(r.grid, r.groups), dim3(r.block), r.lds, s, p, 0);
    return nullptr;
}

// vit: a GEMM of the ViT encoder, which has a tile rule of its own (route_conv)
const char* launch_conv(fav_handle* h, const fav_conv_desc& d, int cout_pad, int ldy, bool vit, const Group& G, hipStream_t s) {
    const Route r = route_conv(d, cout_pad, ldy, vit, G.n);
    if (r.refusal) return r.refusal;
    if (r.kind == ROUTE_PROJ) return launch_proj(h, d, r, G, s);
    ConvParams p;
    p.x = (const uint16_t*)d.x; p.w = (const uint16_t*)d.w; p.bias = d.bias; p.res = (const uint16_t*)d.res; p.y = d.y;
    p.H = d.H; p.W = d.W; p.Cin = d.Cin;
    p.Ho = r.Ho; p.Wo = r.Wo; p.HWo = r.Ho * r.Wo;
    p.Cout = d.Cout; p.ldy = ldy;
    p.kw = d.kw; p.stride = d.stride; p.pad = d.pad;
    p.M = r.M; p.K = r.K; p.nk = r.nk;
    p.relu = d.relu; p.out_f32 = d.out_f32;
    p.tiles_m = r.tiles_m; p.tiles_n = r.tiles_n; p.stage_mid = r.stage_mid;
    p.drop = make_drop(&d.drop);
    p.div_hwo = fastdiv_make((uint32_t)p.HWo);
    p.div_w = fastdiv_make((uint32_t)p.Wo);
    p.dbg = nullptr;
    p.g_x = G.x; p.g_w = G.w; p.g_bias = G.b; p.g_res = G.res; p.g_y = G.y;
    const bool halo = r.kind == ROUTE_CONV_HALO;
    bool lds_ok;
    const HaloKernel kern_halo = halo ? find_kernel(kHaloKernels, r, &lds_ok) : nullptr;
    const ConvKernel kern = halo ? nullptr : find_kernel(kConvKernels, r, &lds_ok);
    if (!kern_halo && !kern) return "conv: no kernel for this route";
    if (!lds_ok) return "conv: cannot reserve LDS for the staged 3x3 kernel";
    const double flops = 2.0 * (double)r.M * d.Cout * r.K * G.n;
    const double bytes = 2.0 * ((double)d.n_frames * d.H * d.W * d.Cin + (double)r.M * d.Cout * (d.res ? 2 : 1) * (d.out_f32 ? 2 : 1)
                                + (double)d.Cout * r.K) * G.n;
    const long long tiles = (long long)r.tiles_m * r.tiles_n;
    const bool dbg_on = FAV_KNOB("FAV_CONV_DBG", 0) != 0;   // experiments build only: per-block phase clocks
    if (dbg_on && !h) { (void)hipMalloc((void**)&p.dbg, (size_t)tiles * 32); (void)hipMemset(p.dbg, 0, (size_t)tiles * 32); }
    auto dbg_report = [&](long long nblocks, int bm, int bn, int bk) {
        if (!p.dbg) return;
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> t((size_t)nblocks * 4);
        (void)hipMemcpy(t.data(), p.dbg, t.size() * 8, hipMemcpyDeviceToHost);
        (void)hipFree(p.dbg);
        unsigned long long lo = ~0ull, hi = 0;
        double ph[3] = {0, 0, 0};
        for (long long i = 0; i < nblocks; ++i) {
            lo = std::min(lo, t[i * 4]); hi = std::max(hi, t[i * 4 + 3]);
            for (int j = 0; j < 3; ++j) ph[j] += (double)(t[i * 4 + j + 1] - t[i * 4 + j]);
        }
        const double span = (double)(hi - lo), life = ph[0] + ph[1] + ph[2];
        fprintf(stderr, "[conv dbg] blocks %lld BMxBNxBK %dx%dx%d span %.1f us; per block: prologue %.2f us, k-loop %.2f us, epilogue %.2f us; "
                        "resident blocks/CU %.2f\n", nblocks, bm, bn, bk, span / 100.0, ph[0] / nblocks / 100.0, ph[1] / nblocks / 100.0,
                ph[2] / nblocks / 100.0, life / span / 256.0);
    };
    Prof pr(h, s, FAV_K_CONV, flops, bytes);
    g_route = r;
    if (halo) hipLaunchKernelGGL(kern_halo, dim3(r.grid, r.groups), dim3(r.block), r.lds, s, p, r.patch_bytes);
    else hipLaunchKernelGGL(kern, dim3(r.grid, r.groups), dim3(r.block), 0, s, p);
    dbg_report(r.grid, halo ? r.a[2] : r.a[0], r.a[1], halo ? 64 : r.a[2]);     // rows x columns x K depth of a tile
    return nullptr;
}

const char* launch_tail(fav_handle* h, const fav_tail_desc& d, const Group& G, hipStream_t s) {
    const Route r = route_tail(d, G.n);
    if (r.refusal) return r.refusal;
    TailParams p = tail_params(r);
    p.t1 = (const uint16_t*)d.x; p.wb = (const uint16_t*)d.wb; p.bias_b = d.bias_b;
    p.wc = (const uint16_t*)d.wc; p.bias_c = d.bias_c; p.res = (const uint16_t*)d.res; p.y = (uint16_t*)d.y;
    p.wa = (const uint16_t*)d.wa; p.bias_a = d.bias_a; p.t1n = (uint16_t*)d.t1n;
    p.drop = make_drop(&d.drop);
    p.g_t1 = G.x; p.g_res = G.res; p.g_y = G.y; p.g_t1n = G.y2;
    p.g_wb = G.wb; p.g_bb = G.bb; p.g_wc = G.w; p.g_bc = G.b; p.g_wa = G.wa; p.g_ba = G.ba;
    p.site_e = d.entry_site;
    bool lds_ok;
    const TailKernel kern = find_kernel(kTailKernels, r, &lds_ok);
    if (!kern) return "bottleneck tail: unsupported shape";
    if (!lds_ok) return "bottleneck tail: cannot reserve LDS";
    const int cmid = d.Cmid, cout = 4 * cmid, nred = r.a[1], bm = r.geom.rp * r.geom.nw;
    const bool has3x3 = r.a[2] != 0;
    const long long M = r.M, nblocks = r.grid;
    const double flops = 2.0 * (double)M * ((has3x3 ? 9.0 * cmid * cmid : 0.0) + (double)cmid * cout + (double)cout * nred) * G.n;
    // res_entry: the residual is the cached tensor [n_img][HW][cout], counted ONCE (every sample's tile re-reads it, from L2), not once per row it serves
    const double res_rows = d.res_entry ? (double)std::min<long long>(d.n_frames, p.drop.n_img) * p.HW : (double)M;
    const double bytes = 2.0 * ((double)M * (cmid + 1.0 * cout + nred) + res_rows * cout + (has3x3 ? 9.0 * cmid * cmid : 0.0) + (double)cmid * cout + (double)cout * nred) * G.n;
    Prof pr(h, s, FAV_K_CONV, flops, bytes);
    const bool dbg_on = FAV_KNOB("FAV_CONV_DBG", 0) != 0;   // experiments build only: per-block phase clocks
    if (dbg_on && !h) { (void)hipMalloc((void**)&p.dbg, (size_t)nblocks * 128); (void)hipMemset(p.dbg, 0, (size_t)nblocks * 128); }
    auto dbg_report = [&]() {
        if (!p.dbg) return;
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> t((size_t)nblocks * 16);
        (void)hipMemcpy(t.data(), p.dbg, t.size() * 8, hipMemcpyDeviceToHost);
        (void)hipFree(p.dbg);
        if (const char* dump = fav_knob_str("FAV_CONV_DBG_DUMP")) {     // raw stamps, [block][16] u64, appended: tools/phase_overlap.py
            if (FILE* f = fopen(dump, "ab")) { const long long hdr[2] = {nblocks, cmid * 1000 + nred}; fwrite(hdr, 8, 2, f); fwrite(t.data(), 8, t.size(), f); fclose(f); }
        }
        unsigned long long lo = ~0ull, hi = 0;
        double ph[5] = {0, 0, 0, 0, 0};
        double cy[5] = {0, 0, 0, 0, 0};   // chunk 1 of wave 0, shader clocks: step A | epilogue | step C | DMA wait | barrier
        double cz[3] = {0, 0, 0};         // ... residual wait at the top of the chunk | requests for the next chunk | the whole chunk (top of 1 to top of 2)
        for (long long i = 0; i < nblocks; ++i) {
            lo = std::min(lo, t[i * 16]); hi = std::max(hi, t[i * 16 + 5]);
            unsigned long long prev = t[i * 16];
            for (int j = 0; j < 5; ++j) { const unsigned long long c = t[i * 16 + j + 1] ? t[i * 16 + j + 1] : prev; ph[j] += (double)(c - prev); prev = c; }
            for (int j = 0; j < 5; ++j) cy[j] += (double)(t[i * 16 + 7 + j] - t[i * 16 + 6 + j]);
            cz[0] += (double)(t[i * 16 + 13] - t[i * 16 + 12]); cz[1] += (double)(t[i * 16 + 6] - t[i * 16 + 13]); cz[2] += (double)(t[i * 16 + 14] - t[i * 16 + 12]);
        }
        const double span = (double)(hi - lo), life = ph[0] + ph[1] + ph[2] + ph[3] + ph[4];
        fprintf(stderr, "[tail dbg] blocks %lld x %d px, Cmid %d Nred %d 3x3 %d: span %.1f us; per block: patch wait %.2f us, 3x3 loop %.2f us, "
                        "T2 + first weights %.2f us, chunks %.2f us, tail %.2f us; resident blocks/CU %.2f\n", nblocks, bm, cmid, nred, (int)has3x3,
                span / 100.0, ph[0] / nblocks / 100.0, ph[1] / nblocks / 100.0, ph[2] / nblocks / 100.0, ph[3] / nblocks / 100.0,
                ph[4] / nblocks / 100.0, life / span / 256.0);
        fprintf(stderr, "[tail dbg]   chunk 1, wave 0, shader clocks: step A %.0f, epilogue %.0f, step C %.0f, DMA wait %.0f, barrier %.0f\n",
                cy[0] / nblocks, cy[1] / nblocks, cy[2] / nblocks, cy[3] / nblocks, cy[4] / nblocks);
        fprintf(stderr, "[tail dbg]   ... residual wait %.0f, next chunk's requests %.0f, whole chunk 1 %.0f\n", cz[0] / nblocks, cz[1] / nblocks, cz[2] / nblocks);
    };
    g_route = r;
    hipLaunchKernelGGL(kern, dim3(r.grid, r.groups), dim3(r.block), r.lds, s, p, r.patch_bytes);
    dbg_report();
    return nullptr;
}

// One work item per thread whenever the grid allows (grid-stride loops only catch the rest): on gfx9
// stores count in vmcnt, so a second iteration's loads would wait for the first iteration's stores.
unsigned grid_for(long long work_items) {
    long long g = (work_items + 255) / 256;
    return (unsigned)std::max<long long>(1, std::min<long long>(g, (1ll << 24) - 1));
}

const char* launch_stem(fav_handle* h, const void* images, int layout, int n, int H, int W, int kh, int kw, int stride, int pad,
                        int kpad, const float* mean, const float* istd, void* out, hipStream_t s) {
    // conv_out truncates towards zero: an empty frame would come out as one output pixel
    if (n < 1 || H < 1 || W < 1) return "stem im2col: n, H and W must be >= 1";
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return "stem im2col: unknown layout";
    if (kh < 1 || kw < 1 || stride < 1 || pad < 0 || H + 2 * pad < kh || W + 2 * pad < kw) return "stem im2col: the window does not fit the padded frame";
    const int Ho = conv_out(H, kh, stride, pad), Wo = conv_out(W, kw, stride, pad);
    const long long total = (long long)n * Ho * Wo * (kpad / 8);
    Prof pr(h, s, FAV_K_STEM, 0.0, (double)n * H * W * 3 * (layout == 0 ? 1 : 4) + (double)total * 16);
    const long long total_pix = (long long)n * Ho * Wo;
    const int ppb = kh <= 64 ? 256 / kh : 0;                    // pixels per block of the row-wise kernel
    const size_t lds = (size_t)ppb * kpad * 2;
    if (ppb >= 4 && lds <= 64 * 1024 && total_pix / ppb < (1ll << 31) - 1) {
        const unsigned blocks = (unsigned)((total_pix + ppb - 1) / ppb);
        if (layout == FAV_LAYOUT_NHWC_U8)
            hipLaunchKernelGGL((stem_im2col_rows_kernel<0>), dim3(blocks), dim3(256), lds, s, images, (uint4*)out, total_pix, H, W, Ho, Wo,
                               kh, kw, stride, pad, kpad, ppb, mean[0], mean[1], mean[2], istd[0], istd[1], istd[2]);
        else
            hipLaunchKernelGGL((stem_im2col_rows_kernel<1>), dim3(blocks), dim3(256), lds, s, images, (uint4*)out, total_pix, H, W, Ho, Wo,
                               kh, kw, stride, pad, kpad, ppb, mean[0], mean[1], mean[2], istd[0], istd[1], istd[2]);
        return nullptr;
    }
    if (layout == FAV_LAYOUT_NHWC_U8)
        hipLaunchKernelGGL((stem_im2col_kernel<0>), dim3(grid_for(total)), dim3(256), 0, s, images, (uint4*)out, n, H, W,
                           Ho, Wo, kh, kw, stride, pad, kpad, mean[0], mean[1], mean[2], istd[0], istd[1], istd[2]);
    else
        hipLaunchKernelGGL((stem_im2col_kernel<1>), dim3(grid_for(total)), dim3(256), 0, s, images, (uint4*)out, n, H, W,
                           Ho, Wo, kh, kw, stride, pad, kpad, mean[0], mean[1], mean[2], istd[0], istd[1], istd[2]);
    return nullptr;
}

const char* launch_maxpool(fav_handle* h, const void* x, void* y, int n, int H, int W, int C, hipStream_t s) {
    // (H + 2 - 3) / 2 + 1 is 1 at H = 0: an empty frame would store a row of -inf
    if (n < 1 || H < 1 || W < 1 || C < 8) return "max pool: n, H and W must be >= 1 and C >= 8";
    const int Ho = conv_out(H, 3, 2, 1), Wo = conv_out(W, 3, 2, 1);
    const long long total = (long long)n * Ho * Wo * (C / 8);
    Prof pr(h, s, FAV_K_MAXPOOL, 0.0, 2.0 * ((double)n * H * W * C + (double)n * Ho * Wo * C));
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const uint4*)x, (uint4*)y, n, H, W,
                       C, Ho, Wo);
    return nullptr;
}

// normalise + 7x7/2 conv (64 channels, weights [64][192]) + bias + ReLU + 3x3/2 max pool, frames -> [n][Hp][Wp][64] bf16
const char* launch_stem_pool(fav_handle* h, const void* images, int layout, int n, int H, int W, const void* w, const float* bias,
                             const float* mean, const float* istd, void* out, const Group& G, hipStream_t s) {
    if (n < 1 || H < 1 || W < 1) return "stem: empty input";
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return "stem: unknown layout";
    StemPoolParams p;
    p.images = images; p.w = (const uint16_t*)w; p.bias = bias; p.out = (uint16_t*)out;
    p.n = n; p.H = H; p.W = W;
    p.Hc = conv_out(H, 7, 2, 3); p.Wc = conv_out(W, 7, 2, 3);
    if (p.Hc < 1 || p.Wc < 1) return "stem: input too small";
    if ((double)H * W * 12.0 >= 2147483647.0) return "stem: frame too large for 32-bit offsets";
    p.Hp = conv_out(p.Hc, 3, 2, 1); p.Wp = conv_out(p.Wc, 3, 2, 1);
    p.tiles_y = (p.Hp + 7) / 8; p.tiles_x = (p.Wp + 7) / 8;
    p.tiles = (long long)n * p.tiles_y * p.tiles_x;
    p.m0 = mean[0]; p.m1 = mean[1]; p.m2 = mean[2]; p.i0 = istd[0]; p.i1 = istd[1]; p.i2 = istd[2];
    p.g_w = G.w; p.g_bias = G.b; p.g_out = G.y;
    const double M = (double)n * p.Hc * p.Wc;
    Prof pr(h, s, FAV_K_CONV, 2.0 * M * 64 * 192 * G.n,
            ((double)n * H * W * 3 * (layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4) + 2.0 * n * p.Hp * p.Wp * 64 + 2.0 * 64 * 192) * G.n);
    // two blocks per CU (232 VGPRs, 66 KB of LDS); blocks loop over the tiles with the weights in registers
    const unsigned blocks = (unsigned)std::min<long long>(p.tiles, std::max(1, 256 * 2 / G.n));
    route_set(ROUTE_STEM_POOL, layout == FAV_LAYOUT_NHWC_U8 ? 0 : 1);
    if (layout == FAV_LAYOUT_NHWC_U8) hipLaunchKernelGGL(stem7_pool_kernel<0>, dim3(blocks, G.n), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(stem7_pool_kernel<1>, dim3(blocks, G.n), dim3(256), 0, s, p);
    return nullptr;
}

const char* launch_avgpool(fav_handle* h, const void* x, void* y, int n, int HW, int C, const fav_dropout_desc* drop, const Group& G,
                           hipStream_t s) {
    if (n < 1 || HW < 1 || C < 16) return "average pool: n and HW must be >= 1 and C >= 16";
    if (const char* e = check_drop("average pool", drop, n)) return e;
    const DropParams dp = make_drop(drop);
    const long long total = (long long)n * (C / 16);
    Prof pr(h, s, FAV_K_AVGPOOL, 0.0, 2.0 * ((double)n * HW * C + (double)n * C));
    const float inv = 1.0f / (float)HW;
    hipLaunchKernelGGL(avgpool_kernel, dim3(grid_for(total), G.n), dim3(256), 0, s, (const uint4*)x, (uint4*)y, n, HW, C, inv,
                       dp, G.x, G.y);
    return nullptr;
}

const char* launch_entry_dropout(fav_handle* h, const void* x, void* out, long long elems, int n_out, const fav_dropout_desc* drop,
                                 hipStream_t s) {
    if (!drop || drop->site < 0) return "entry dropout: needs a dropout site";
    if (elems < 16 || n_out < 1) return "entry dropout: elems_per_frame must be >= 16 and n_out >= 1";
    if (const char* e = check_drop("entry dropout", drop, n_out)) return e;
    const DropParams dp = make_drop(drop);
    const long long total = (elems / 16) * std::min<long long>(dp.n_img, n_out);   // threads: one per cached chunk
    Prof pr(h, s, FAV_K_DROPOUT, 0.0, 2.0 * (double)elems * (n_out + std::min<long long>(dp.n_img, n_out)));
    hipLaunchKernelGGL(entry_dropout_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const uint4*)x, (uint4*)out,
                       elems / 16, n_out, dp);
    return nullptr;
}

// Entry dropout + the 1x1 reduce behind it (entry_reduce_kernel); entry_reduce_supported: fav_plan.hpp
const char* launch_entry_reduce(fav_handle* h, const void* x, void* y, const void* wa, const float* bias_a, void* t1, int C, int nred,
                                int HW, int n_out, const fav_dropout_desc* drop, hipStream_t s) {
    if (!drop || drop->site < 0 || n_out < 1 || HW < 1) return "entry reduce: needs a dropout site, n_out >= 1 and HW >= 1";
    if (const char* e = check_drop("entry reduce", drop, n_out)) return e;
    const DropParams dp = make_drop(drop);
    if (!entry_reduce_supported(C, nred, dp.n_img, HW)) return "entry reduce: unsupported shape";
    EntryReduceParams p;
    p.x = (const uint16_t*)x; p.y = (uint16_t*)y; p.wa = (const uint16_t*)wa; p.bias_a = bias_a; p.t1 = (uint16_t*)t1;
    p.HW = HW; p.M = (int)((long long)dp.n_img * HW); p.n_out = n_out;
    p.drop = dp;
    p.div_hw = fastdiv_make((uint32_t)HW);
    const long long cached = std::min<long long>(dp.n_img, n_out);
    const double rows = (double)n_out * HW;
    Prof pr(h, s, FAV_K_CONV, 2.0 * rows * C * nred, 2.0 * ((double)cached * HW * C + rows * ((y ? C : 0) + nred) + (double)C * nred));
    route_set(ROUTE_ENTRY_REDUCE, 256, 64);
    hipLaunchKernelGGL((entry_reduce_kernel<256, 64>), dim3((unsigned)((p.M + 127) / 128)), dim3(256), 0, s, p);
    return nullptr;
}

// The conformal prediction-set head's arguments (fav_classify_sets / fav_conformal_scores / fav_op_head_sets): cp checked
// by check_conformal; rec and / or (true_labels, true_scores).
struct HeadSets {
    const fav_conformal* cp;
    int64_t first_index;
    const int32_t* true_labels;
    float* true_scores;
    fav_pred_set* rec;
};

const char* check_conformal(const fav_conformal* cp) {
    if (!cp || cp->struct_size != sizeof(fav_conformal)) return "conformal: cp is NULL or its struct_size is wrong";
    if (cp->score_kind != FAV_CP_LAC && cp->score_kind != FAV_CP_APS) return "conformal: unknown score_kind";
    if (std::isnan(cp->qhat)) return "conformal: qhat is NaN";
    if (!(cp->lambda >= 0.f) || !std::isfinite(cp->lambda)) return "conformal: lambda must be finite and >= 0";
    if (cp->k_reg < 0) return "conformal: k_reg must be >= 0";
    if (cp->randomized != 0 && cp->randomized != 1) return "conformal: randomized must be 0 or 1";
    if (cp->score_kind == FAV_CP_LAC && (cp->randomized || cp->lambda != 0.f))
        return "conformal: FAV_CP_LAC takes neither randomized nor lambda";
    return nullptr;
}

// The temperature-sweep head's arguments (fav_classify_sweep / fav_op_head_sweep): K temperatures on the host, the frames'
// true labels and the [n][K] cells on the device.
struct HeadSweep {
    const float* temps;
    int32_t K;
    const int32_t* true_labels;
    fav_calib_cell* cells;
};

// Everything about a sweep that can be wrong without looking at the device (NULL: nothing).  T < 0: not known yet (the
// classify entry point checks the handle's configuration instead).
const char* check_sweep(const HeadSweep& sw, int C, int T, int kind) {
    if (sw.K < 1 || sw.K > FAV_SWEEP_MAX_TEMPS) return "sweep: K must be in [1, 32] (FAV_SWEEP_MAX_TEMPS)";
    if (!sw.temps) return "sweep: temperatures are NULL";
    for (int k = 0; k < sw.K; ++k)
        if (!std::isfinite(sw.temps[k]) || !(sw.temps[k] > 0.f)) return "sweep: every temperature must be finite and > 0";
    if (!sw.cells || ((uintptr_t)sw.cells & 7)) return "sweep: cells must be non-NULL and 8-byte aligned";
    if (!sw.true_labels) return "sweep: true labels are NULL";
    if (C > 1024 || C < 1) return "head: num_classes must be in [1, 1024]";
    if (kind < 0 || kind > 2) return "sweep: conf_kind must be 0, 1 or 2";
    if (kind == FAV_CONF_MUTUAL_INFO && ((T >= 0 && T < 2) || C < 2))
        return "sweep: conf_kind 2 (mutual information) needs T >= 2 samples and num_classes >= 2";
    return nullptr;
}

// the class-probability head (fav_curve.hpp): pbar of classes[i] (NULL: of the frame's label) to prob, the label to labels (may be NULL)
struct HeadClassProb {
    const int32_t* classes;
    float* prob;
    int32_t* labels;
};

// What the head writes: labels and conf out_stride elements apart (2: interleaved records), the optional failure flags and
// scores, and at most one of rec (one fav_uncertainty per frame), sets, sweep and cprob.  The public entry points build it;
// classify_gate and classify_on_stream pass it through.
struct HeadOut {
    int32_t* labels = nullptr;
    float* conf = nullptr;
    uint8_t* fail = nullptr;
    float* score = nullptr;
    int out_stride = 1;
    fav_uncertainty* rec = nullptr;
    const HeadSets* sets = nullptr;
    const HeadSweep* sweep = nullptr;
    const HeadClassProb* cprob = nullptr;
};

// rec (one fav_uncertainty per frame) or conf_kind FAV_CONF_MUTUAL_INFO: head_unc_kernel; sets: head_sets_kernel;
// sweep: head_sweep_kernel (temperature, tau, labels .. score are then not used); cprob: head_class_prob_kernel (kind, tau,
// labels .. score are not used); otherwise head_kernel
const char* launch_head(fav_handle* h, const float* logits, int T, int n, int C, int ld, float temperature, int kind,
                        float tau, const HeadOut& out, hipStream_t s) {
    const HeadSets* const sets = out.sets;
    const HeadSweep* const sweep = out.sweep;
    if (sweep)
        if (const char* e = check_sweep(*sweep, C, T, kind)) return e;
    if (C > 1024 || C < 1) return "head: num_classes must be in [1, 1024]";
    if (ld % 4 != 0 || ld < C) return "head: bad row stride";
    const float inv_temp = 1.0f / temperature;
    const float inv_lnC = C > 1 ? (float)(1.0 / std::log((double)C)) : 0.f;
    const int K = std::min(C, T);           // largest mutual information of T samples over C classes: ln K
    const float inv_lnK = K > 1 ? (float)(1.0 / std::log((double)K)) : 0.f;
    // one block per frame; the instantiation by the class count (NV = 1: up to 256 classes, 4: up to 1024)
#define FAV_LAUNCH_HEAD(KERNEL, LDS, ...)                                                                                   \
    do {                                                                                                                    \
        if (C <= 256)                                                                                                       \
            hipLaunchKernelGGL((KERNEL<1>), dim3(n), dim3(256), LDS, s, logits, T, n, C, ld, inv_temp, kind, tau, inv_lnC,  \
                               __VA_ARGS__);                                                                                \
        else                                                                                                                \
            hipLaunchKernelGGL((KERNEL<4>), dim3(n), dim3(256), LDS, s, logits, T, n, C, ld, inv_temp, kind, tau, inv_lnC,  \
                               __VA_ARGS__);                                                                                \
    } while (0)
    if (sweep) {
        if (T < 1 || T > 4096) return "head: the sweep head takes 1 <= T <= 4096 samples";
        SweepParams p;
        for (int k = 0; k < kSweepMaxTemps; ++k) p.inv_temp[k] = 1.0f / sweep->temps[std::min(k, sweep->K - 1)];
        p.K = sweep->K;
        // dynamic LDS: as many of the frame's rows as fit beside the kernel's 16.4 KB of static LDS
        const int kSweepLds = 140 * 1024;
        const int row_bytes = ((C + 3) & ~3) * 4;
        p.t_lds = std::min(T, kSweepLds / row_bytes);
        const size_t lds = (size_t)p.t_lds * row_bytes;
        // bytes: the logits once, the labels, the cells
        Prof pr(h, s, FAV_K_HEAD, 0.0, 4.0 * (double)T * n * C + 4.0 * n + 16.0 * n * sweep->K);
#define FAV_LAUNCH_SWEEP(NV_)                                                                                               \
    do {                                                                                                                    \
        static DeviceFlags attr_set;   /* hipFuncSetAttribute applies to the CURRENT device only */                         \
        if (!attr_set.test_current()) {                                                                                     \
            if (hipFuncSetAttribute((const void*)head_sweep_kernel<NV_>, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                    kSweepLds) != hipSuccess)                                                               \
                return "head: cannot reserve LDS for the sweep head";                                                       \
            attr_set.set_current();                                                                                         \
        }                                                                                                                   \
        hipLaunchKernelGGL((head_sweep_kernel<NV_>), dim3(n), dim3(256), lds, s, logits, T, n, C, ld, kind, inv_lnC,        \
                           inv_lnK, p, sweep->true_labels, (int*)sweep->cells);                                             \
    } while (0)
        if (C <= 256) FAV_LAUNCH_SWEEP(1); else FAV_LAUNCH_SWEEP(4);
#undef FAV_LAUNCH_SWEEP
    } else if (sets) {
        if (const char* e = check_conformal(sets->cp)) return e;
        if (!sets->rec && !sets->true_labels) return "head: the sets head needs records or calibration labels";
        if (!sets->true_labels != !sets->true_scores) return "head: true_labels and true_scores go together";
        if ((uintptr_t)sets->rec & 7) return "head: prediction-set records must be 8-byte aligned";
        if (sets->first_index < 0 || sets->first_index + n > 0xFFFFFFFFll) return "head: first_image_index out of range";
        SetsParams p;
        p.score_kind = sets->cp->score_kind; p.randomized = sets->cp->randomized; p.k_reg = sets->cp->k_reg;
        p.lambda = sets->cp->lambda; p.qhat = sets->cp->qhat;
        p.seed_lo = (uint32_t)(sets->cp->seed & 0xFFFFFFFFull); p.seed_hi = (uint32_t)(sets->cp->seed >> 32);
        p.first_index = sets->first_index;
        // bytes: the logits, the labels and scores of a calibration call, the outputs
        Prof pr(h, s, FAV_K_HEAD, 0.0, 4.0 * (double)T * n * C + (sets->true_labels ? 8.0 : 0.0) * n +
                                       (sets->rec ? 160.0 : 0.0) * n + (out.fail ? 1.0 : 0.0) * n + (out.score ? 4.0 : 0.0) * n);
        FAV_LAUNCH_HEAD(head_sets_kernel, 0, inv_lnK, p, sets->true_labels, sets->true_scores, (int*)sets->rec, out.fail, out.score);
    } else if (out.cprob) {
        if (T < 1 || T > 4096) return "head: the class-probability head takes 1 <= T <= 4096 samples";
        if (!out.cprob->prob || (((uintptr_t)out.cprob->prob | (uintptr_t)out.cprob->classes | (uintptr_t)out.cprob->labels) & 3))
            return "head: prob must be non-NULL; prob, classes and labels 4-byte aligned";
        Prof pr(h, s, FAV_K_HEAD, 0.0, 4.0 * (double)T * n * C + 12.0 * n);
        if (C <= 256)
            hipLaunchKernelGGL((head_class_prob_kernel<1>), dim3(n), dim3(256), 0, s, logits, T, n, C, ld, inv_temp, out.cprob->classes,
                               out.cprob->prob, out.cprob->labels);
        else
            hipLaunchKernelGGL((head_class_prob_kernel<4>), dim3(n), dim3(256), 0, s, logits, T, n, C, ld, inv_temp, out.cprob->classes,
                               out.cprob->prob, out.cprob->labels);
    } else if (out.rec || kind == FAV_CONF_MUTUAL_INFO) {
        if (T < 1 || T > 4096) return "head: the uncertainty head takes 1 <= T <= 4096 samples";
        // bytes: the logits, the second pass's p_t[label] reloads, the outputs
        Prof pr(h, s, FAV_K_HEAD, 0.0, 4.0 * (double)T * n * C + 4.0 * (double)T * n + (out.rec ? 72.0 : 8.0) * n);
        // dynamic LDS: per-sample max and 1/sum
        FAV_LAUNCH_HEAD(head_unc_kernel, (size_t)T * 8, inv_lnK, out.labels, out.conf, out.fail, out.score, out.out_stride, (int*)out.rec);
    } else {
        Prof pr(h, s, FAV_K_HEAD, 0.0, 4.0 * (double)T * n * C + 8.0 * n);
        FAV_LAUNCH_HEAD(head_kernel, 0, out.labels, out.conf, out.fail, out.score, out.out_stride);
    }
#undef FAV_LAUNCH_HEAD
    return nullptr;
}

// ------------------------------------------------------------------ ViT launchers
const char* launch_layernorm(fav_handle* h, const void* x, long long ldx, const float* gamma, const float* beta, void* y, long long rows,
                             int D, float eps, hipStream_t s) {
    if (D % 4 != 0 || D > 1024 || rows < 1) return "layernorm: need D % 4 == 0, D <= 1024";
    Prof pr(h, s, FAV_K_AVGPOOL, 0.0, (double)rows * D * 4);
    const int lnr = (int)FAV_KNOB("FAV_LN_ROWS", 4);    // rows per wave (experiments build: 1 / 2 / 4)
    if (rows >= 4096 && lnr >= 4)
        hipLaunchKernelGGL(layernorm_kernel<4>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, (const uint16_t*)x, ldx, gamma, beta,
                           (uint16_t*)y, rows, D, eps);
    else if (rows >= 4096 && lnr >= 2)
        hipLaunchKernelGGL(layernorm_kernel<2>, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, (const uint16_t*)x, ldx, gamma, beta,
                           (uint16_t*)y, rows, D, eps);
    else
        hipLaunchKernelGGL(layernorm_kernel<1>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const uint16_t*)x, ldx, gamma, beta,
                           (uint16_t*)y, rows, D, eps);
    return nullptr;
}

// ---- chained stream-K GEMM (gemm_streamk_kernel): the ViT encoder's linear layers -----------------------------------------------
// Returns false when the shape is not the kernel's (the caller then takes the tile-per-block kernel: same bits).
// The grid is k x CUs workgroups, k = 3, 2 or 1: the largest for which every XCD group's share of the tiles is >= its workgroups,
// i.e. every workgroup's share of K steps is at least one whole tile (a workgroup then publishes at most one partial accumulator,
// at its start, and takes over at most one, at its end).
struct SkDevice { fav_handle::SkWs ws; int device = -1; };
bool sk_prepare(fav_handle::SkWs* w, int grid) {
    if (w->grid_cap >= grid) return true;
    if (w->ws) { (void)hipFree(w->ws); (void)hipFree(w->flags); (void)hipFree(w->err); w->ws = nullptr; }
    const int cap = std::max(grid, 768);
    if (hipMalloc((void**)&w->ws, (size_t)cap * 65536) != hipSuccess || hipMalloc((void**)&w->flags, (size_t)cap * 4) != hipSuccess ||
        hipMalloc((void**)&w->err, 4) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMemset(w->flags, 0, (size_t)cap * 4) != hipSuccess || hipMemset(w->err, 0, 4) != hipSuccess) return false;
    w->grid_cap = cap;
    w->epoch = 0;
    return true;
}
// Off by default: bit-identical to the tile-per-block kernel but slower at the encoder's shapes on this part (profiles/r4g_streamk_*:
// the hand-offs' agent-scope fences and 2 x 64 KB per workgroup cost ~25 % of a launch, and shares that start at different K steps
// lose the lock step that keeps the tile kernel's LDS-DMA stream in the XCD's 4 MB L2).  FAV_STREAMK=1 routes the encoder through it.
bool streamk_enabled() {
    return FAV_KNOB("FAV_STREAMK", 0) != 0;
}
bool launch_gemm_streamk(fav_handle* h, const void* a, const void* w, const float* bias, const void* res, void* y, long long M, int K, int N,
                         int act, hipStream_t s) {
    if ((h && !streamk_enabled()) || M < 1 || K % 32 != 0 || K < 128 || N % 128 != 0 || act < 0 || act > 2) return false;
    const long long tiles_m = (M + 127) / 128;
    const long long tiles = tiles_m * (N / 128);
    if ((double)(M + 128) * std::max(N, K) * 2.0 >= 2147483647.0 || (double)N * K * 2.0 >= 2147483647.0 || tiles > 0x3fffffffLL) return false;
    static int n_cu = 0;
    if (!n_cu) { int dev = 0; hipDeviceProp_t prop; if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false; n_cu = prop.multiProcessorCount; }
    int per_cu = 0;
    for (int k = 3; k >= 1; --k)
        if (tiles / 8 >= (long long)(n_cu * k) / 8) { per_cu = k; break; }
    if (!per_cu || (n_cu * per_cu) % 8 != 0) return false;
    const int grid = n_cu * per_cu;
    static SkDevice op_ws[16];               // op-level calls (no handle): one workspace per device, kept for the life of the process
    fav_handle::SkWs* W;
    if (h) W = &h->sk[h->sk_slot];
    else { int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false; W = &op_ws[dev].ws; }
    if (!sk_prepare(W, grid)) return false;
    GemmSkParams p;
    memset(&p, 0, sizeof p);
    p.a = (const uint16_t*)a; p.w = (const uint16_t*)w; p.bias = bias; p.res = (const uint16_t*)res; p.y = (uint16_t*)y;
    p.M = (int)M; p.N = N; p.K = K; p.ksteps = K / 32;
    p.tiles_n = N / 128; p.tiles = (int)tiles;
    p.act = act;
    if (FAV_KNOB("FAV_SK_NOHANDOFF", 0) != 0) p.act |= 0x100;   // experiments build, TIMING ONLY (wrong results): what the hand-offs cost
    p.Q = grid / 8;
    p.ws = W->ws; p.flags = W->flags; p.err = W->err;
    p.epoch = ++W->epoch;
    if (p.epoch == 0) { (void)hipMemsetAsync(W->flags, 0, (size_t)W->grid_cap * 4, s); p.epoch = W->epoch = 1; }
    p.div_tn = fastdiv_make((uint32_t)p.tiles_n);
    const double flops = 2.0 * (double)M * N * K;
    const double bytes = 2.0 * ((double)M * K + (double)M * N * (res ? 2 : 1) + (double)N * K);
    Prof pr(h, s, FAV_K_CONV, flops, bytes);
    // dynamic LDS the kernel never touches: it makes per_cu workgroups - not more - fit a CU beside the kernel's own 53 248 B, so the
    // smaller grids sit two / one per CU instead of three on some CUs and none on others
    const int pad_lds = per_cu == 3 ? 0 : (per_cu == 2 ? 26 * 1024 : 104 * 1024);
    static DeviceFlags attr_set;
    if (!attr_set.test_current()) {
        if (hipFuncSetAttribute((const void*)gemm_streamk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 104 * 1024) != hipSuccess) { (void)hipGetLastError(); return false; }
        attr_set.set_current();
    }
    const bool dbg_on = FAV_KNOB("FAV_SK_DBG", 0) != 0;   // experiments build only: where a step's ticks go
    if (dbg_on && !h) { (void)hipMalloc((void**)&p.dbg, (size_t)grid * 64); (void)hipMemset(p.dbg, 0, (size_t)grid * 64); }
    hipLaunchKernelGGL(gemm_streamk_kernel, dim3((unsigned)grid), dim3(256), pad_lds, s, p);
    if (p.dbg) {
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> t((size_t)grid * 8);
        (void)hipMemcpy(t.data(), p.dbg, t.size() * 8, hipMemcpyDeviceToHost);
        (void)hipFree(p.dbg);
        double ph[5] = {0, 0, 0, 0, 0}, steps = 0;
        unsigned long long lo = ~0ull, hi = 0; double life = 0;
        for (int i = 0; i < grid; ++i) {
            for (int k = 0; k < 5; ++k) ph[k] += (double)t[i * 8 + k];
            steps += (double)t[i * 8 + 5];
            lo = std::min(lo, t[i * 8 + 6]); hi = std::max(hi, t[i * 8 + 7]); life += (double)(t[i * 8 + 7] - t[i * 8 + 6]);
        }
        fprintf(stderr, "[sk dbg] span %.1f us, mean workgroup life %.1f us, resident workgroups per CU %.2f\n", (hi - lo) / 100.0, life / grid / 100.0, life / (double)(hi - lo) / n_cu);
        fprintf(stderr, "[sk dbg] M %lld K %d N %d grid %d: %.1f steps per workgroup; ticks per step (wave 0): stage %.0f, reads + MFMAs %.0f, segment end %.0f, "
                        "vmcnt wait %.0f, barrier %.0f\n", M, K, N, grid, steps / grid, ph[0] / steps, ph[1] / steps, ph[2] / steps, ph[3] / steps, ph[4] / steps);
    }
    return true;
}

const char* launch_attention(fav_handle* h, const void* qkv, void* out, int n, int T, int D, int heads, int math_mode, hipStream_t s) {
    const Route r = route_attention(n, T, D, heads, math_mode);
    if (r.refusal) return r.refusal;
    bool lds_ok;
    const AttnKernel kern = find_kernel(kAttnKernels, r, &lds_ok);
    if (!kern) return "attention: no kernel for this route";
    if (!lds_ok) return "attention: cannot reserve LDS";
    const double flops = 4.0 * n * heads * (double)T * T * 64;
    Prof pr(h, s, FAV_K_CONV, flops, (double)n * T * D * 2 * 4);
    g_route = r;
    hipLaunchKernelGGL(kern, dim3(r.grid), dim3(r.block), r.lds, s, (const uint16_t*)qkv, (uint16_t*)out, T, D, heads);
    return nullptr;
}

void launch_vit_assemble(fav_handle* h, const void* emb, const float* pos, void* x, int n, int ntok, int D, hipStream_t s) {
    const long long total = (long long)n * ntok * (D / 4);
    Prof pr(h, s, FAV_K_STEM, 0.0, (double)n * ntok * D * 4);
    hipLaunchKernelGGL(vit_assemble_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const uint16_t*)emb, pos, (uint16_t*)x, n, ntok, D);
}

// ------------------------------------------------------------------ workspace
// Everything the plan needs on the device, allocated once.  ResNet archs: five rotating buffers and the im2col matrix sized
// for the largest (chunk x tensor) in any phase, the output of each phase but the last, the logits, one lane per member.
fav_status alloc_workspace(fav_handle* h) {
    const fav_config& c = h->cfg;
    const Plan& P = h->plan;
    h->weights.resize(P.layers.size());
    if (h->vit) {
        const VitDef& V = kVit[c.arch - 2];
        const size_t B = (size_t)c.max_batch, D = (size_t)V.dim, ntok = (size_t)P.ntok, np = ntok - 1;
        HIP_TRY(h, hipMalloc(&h->v_patches, B * np * (size_t)(V.patch * V.patch * 3) * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_emb, B * np * D * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_x, B * ntok * D * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_y, B * ntok * D * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_qkv, B * ntok * 3 * D * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_hid, B * ntok * (size_t)V.mlp * 2 + 256));
        HIP_TRY(h, hipMalloc(&h->v_cls, B * D * 2 + 256));
        HIP_TRY(h, hipMalloc((void**)&h->logits, B * P.cpad * 4 + 256));
        return FAV_OK;
    }
    const long long nv_max = (long long)c.max_batch * P.T_eff;
    const size_t nph = P.phases.size();
    size_t act_bytes = 0, a1_bytes = 0;
    for (const Phase& p : P.phases) {
        for (int k = p.op_begin; k < p.op_end; ++k) {
            const Op& o = P.ops[k];
            const size_t b = (size_t)o.out_elems * (o.out_f32 ? 4 : 2) * p.chunk;
            if (o.out == B_A1) a1_bytes = std::max(a1_bytes, b);
            else if (o.out >= 0) act_bytes = std::max(act_bytes, b);
        }
    }
    act_bytes = (act_bytes + 255) / 256 * 256 + 256;
    a1_bytes = (a1_bytes + 255) / 256 * 256 + 256;
    // every workspace tensor is a slab of n_members equal parts, so that a grouped launch finds member g's tensors at a constant stride
    const size_t parts = (size_t)h->n_members;
    for (int i = 0; i < 5; ++i) HIP_TRY(h, hipMalloc(&h->act[i], act_bytes * parts));
    h->act_bytes = act_bytes;
    HIP_TRY(h, hipMalloc(&h->a1, a1_bytes * parts));
    h->a1_bytes = a1_bytes;
    h->phase_out.assign(nph, nullptr);
    std::vector<size_t> phase_bytes(nph, 0);
    for (size_t i = 0; i + 1 < nph; ++i) {
        const Phase& p = P.phases[i];
        const long long dom = p.suffix ? nv_max : c.max_batch;
        phase_bytes[i] = ((size_t)dom * p.out_elems * p.out_bytes_per_elem + 255) / 256 * 256 + 256;
        HIP_TRY(h, hipMalloc(&h->phase_out[i], phase_bytes[i] * parts));
    }
    HIP_TRY(h, hipMalloc((void**)&h->logits, (size_t)nv_max * h->n_members * P.cpad * 4 + 256));
    h->lanes.resize(h->n_members);
    if (h->n_members > 1) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_members, hipEventDisableTiming));
    for (int m = 0; m < h->n_members; ++m) {
        Lane& w = h->lanes[m];
        w.member = m;
        if (h->n_members > 1) {     // a single model runs on the caller's stream
            HIP_TRY(h, hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
            HIP_TRY(h, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
        }
        for (int i = 0; i < 5; ++i) w.act[i] = (char*)h->act[i] + (size_t)m * act_bytes;
        w.a1 = (char*)h->a1 + (size_t)m * a1_bytes;
        for (size_t i = 0; i + 1 < nph; ++i) w.phase_out[i] = (char*)h->phase_out[i] + (size_t)m * phase_bytes[i];
    }
    return FAV_OK;
}

// ------------------------------------------------------------------ execution
// Virtual frames [v_begin, v_end) of phase pi on the lane's stream, in the lane's workspace, with the lane's member's weights;
// lane.groups > 1: every op one launch over that many members.  Member m writes logits[m][n][cpad]: the head then averages
// members exactly as it averages samples.
fav_status run_chunks(fav_handle* h, size_t pi, const Frames& f, const Lane& lane, long long v_begin, long long v_end) {
    const fav_config& c = h->cfg;
    const Phase& p = h->plan.phases[pi];
    const hipStream_t s = lane.stream;
    const int n = f.n, layout = f.layout;
    auto LW = [&](int li) -> void* { return h->weights[li].w_m[lane.member]; };
    auto LB = [&](int li) -> float* { return h->weights[li].b_m[lane.member]; };
    const size_t logits_slot = (size_t)n * h->plan.cpad * 4;     // one member's part of the logits in a call of n frames
    const bool last = pi + 1 == h->plan.phases.size();
    const char* pin_base = pi == 0 ? (const char*)f.images : (const char*)lane.phase_out[pi - 1];
    const int in_bpe = pi == 0 ? (layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4) : h->plan.phases[pi - 1].out_bytes_per_elem;
    // a suffix phase that follows the prefix reads frame (v % n); later phases read virtual frame v
    const bool in_is_virtual = pi > 0 && h->plan.phases[pi - 1].suffix;
    char* pout_base = last ? (char*)h->logits + (size_t)lane.member * logits_slot : (char*)lane.phase_out[pi];
    const uint32_t thr = (uint32_t)std::lround((double)c.dropout_p * 256.0);
    const float scale = thr > 0 ? (float)(1.0 / (1.0 - thr / 256.0)) : 1.0f;
    float istd[3] = {1.0f / c.stdev[0], 1.0f / c.stdev[1], 1.0f / c.stdev[2]};

    for (long long v0 = v_begin; v0 < v_end; v0 += p.chunk) {
        const int cn = (int)std::min<long long>(p.chunk, v_end - v0);
        auto buf = [&](int id, const Op& o) -> void* {
            switch (id) {
                case B_INPUT: return (void*)(pin_base + (size_t)v0 * o.in_elems * in_bpe);
                case B_PHASE_IN:
                    if (!in_is_virtual && p.suffix) return (void*)pin_base;  // entry dropout indexes v % n itself
                    return (void*)(pin_base + (size_t)v0 * p.in_elems * in_bpe);
                case B_PHASE_OUT: return (void*)(pout_base + (size_t)v0 * p.out_elems * p.out_bytes_per_elem);
                case B_A1: return lane.a1;
                case B_NONE: return nullptr;
                default: return lane.act[id];
            }
        };
        // grouped launch: byte stride from this lane's tensor to the next member's, per buffer and per layer
        auto gbuf = [&](int id) -> long long {
            const Lane& next = h->lanes[lane.member + 1];
            switch (id) {
                case B_INPUT: case B_NONE: return 0;
                case B_PHASE_IN: return pi == 0 ? 0 : (char*)next.phase_out[pi - 1] - (char*)lane.phase_out[pi - 1];
                case B_PHASE_OUT: return last ? (long long)logits_slot : (char*)next.phase_out[pi] - (char*)lane.phase_out[pi];
                case B_A1: return (char*)next.a1 - (char*)lane.a1;
                default: return (char*)next.act[id] - (char*)lane.act[id];
            }
        };
        auto gw = [&](int li) -> long long { return li >= 0 ? (long long)h->weights[li].w_stride : 0; };
        auto gb = [&](int li) -> long long { return li >= 0 ? (long long)h->weights[li].b_stride : 0; };
        for (int k = p.op_begin; k < p.op_end; ++k) {
            const Op& o = h->plan.ops[k];
            h->cur_op = k;
            Group G;
            if (lane.groups > 1) {
                G.n = lane.groups;
                G.x = gbuf(o.in); G.res = gbuf(o.res); G.y = gbuf(o.out); G.y2 = gbuf(o.out2);
                if (o.kind == OP_TAIL) { G.w = gw(o.layer_c); G.b = gb(o.layer_c); G.wb = gw(o.layer); G.bb = gb(o.layer); G.wa = gw(o.layer_a); G.ba = gb(o.layer_a); }
                else { G.w = gw(o.layer); G.b = gb(o.layer); }
            }
            fav_dropout_desc dd;
            dd.site = o.site; dd.threshold = thr; dd.scale = scale; dd.seed = c.seed;
            dd.v0 = p.suffix ? v0 : 0; dd.n_img = n; dd.first_image_index = f.first_index;
            const bool stage_here = h->stage_tap.on && k == h->stage.op;
            switch (o.kind) {
                case OP_STEM_IM2COL: {
                    const LayerShape& L = h->plan.layers[o.layer];
                    if (const char* e = launch_stem(h, buf(o.in, o), layout, cn, o.H, o.W, L.kh, L.kw, L.stride, L.pad, L.k, c.mean,
                                                    istd, buf(o.out, o), s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                }
                case OP_CONV: {
                    const LayerShape& L = h->plan.layers[o.layer];
                    fav_conv_desc d;
                    d.x = buf(o.in, o); d.w = LW(o.layer); d.bias = LB(o.layer); d.res = buf(o.res, o); d.y = buf(o.out, o);
                    d.n_frames = cn; d.H = o.H; d.W = o.W; d.Cin = o.C; d.Cout = L.cout;
                    // the stem GEMM runs as a 1x1 conv over the im2col matrix
                    const bool stem = (o.in == B_A1);
                    d.kh = stem ? 1 : L.kh; d.kw = stem ? 1 : L.kw; d.stride = stem ? 1 : L.stride; d.pad = stem ? 0 : L.pad;
                    d.relu = o.relu; d.out_f32 = o.out_f32; d.math_mode = c.math_mode;
                    d.drop = dd;
                    const int ldy = o.out_f32 ? L.cout_pad : L.cout;
                    if (h->tap && last && k + 1 == p.op_end) {
                        // the feature tap: the rows the fc reads, to [member][virtual frame] of feat_buf, in front of the launch
                        const size_t row = (size_t)o.C * 2, member_rows = (size_t)n * (p.suffix ? h->plan.T_eff : 1);
                        for (int g = 0; g < lane.groups; ++g)
                            HIP_TRY(h, hipMemcpyAsync((char*)h->feat_buf + ((size_t)(lane.member + g) * member_rows + (size_t)v0) * row,
                                                      (const char*)d.x + (long long)g * G.x, (size_t)cn * row, hipMemcpyDeviceToDevice, s));
                    }
                    if (const char* e = launch_conv(h, d, L.cout_pad, ldy, false, G, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                }
                case OP_TAIL: {
                    fav_tail_desc d;
                    memset(&d, 0, sizeof d);
                    d.x = buf(o.in, o);
                    if (o.layer >= 0) { d.wb = LW(o.layer); d.bias_b = LB(o.layer); }
                    d.wc = LW(o.layer_c); d.bias_c = LB(o.layer_c); d.res = buf(o.res, o); d.y = buf(o.out, o);
                    if (o.layer_a >= 0) { d.wa = LW(o.layer_a); d.bias_a = LB(o.layer_a); d.t1n = buf(o.out2, o); }
                    d.n_frames = cn; d.H = o.H; d.W = o.W; d.Cmid = o.C; d.Nred = o.Co2;
                    d.drop = dd;
                    if (o.res_entry) { d.res = pin_base; d.res_entry = 1; d.entry_site = h->plan.first_site; }   // the cached prefix output
                    if (const char* e = launch_tail(h, d, G, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                }
                case OP_STEM_POOL:
                    if (const char* e = launch_stem_pool(h, buf(o.in, o), layout, cn, o.H, o.W, LW(o.layer), LB(o.layer), c.mean, istd,
                                                         buf(o.out, o), G, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                case OP_MAXPOOL:
                    if (const char* e = launch_maxpool(h, buf(o.in, o), buf(o.out, o), cn, o.H, o.W, o.C, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                case OP_AVGPOOL:
                    if (h->map_tap.on) {
                        // the map tap: the frames the pool reads, to [virtual frame] of its buffer, in front of the launch
                        const size_t frame = (size_t)o.H * o.W * o.C * 2;
                        HIP_TRY(h, hipMemcpyAsync((char*)h->map_tap.buf + (size_t)v0 * frame, buf(o.in, o), (size_t)cn * frame,
                                                  hipMemcpyDeviceToDevice, s));
                    }
                    if (stage_here) {
                        // the stage tap at stage 4: the same frames, to its own buffer
                        const size_t frame = (size_t)o.H * o.W * o.C * 2;
                        HIP_TRY(h, hipMemcpyAsync((char*)h->stage_tap.buf + (size_t)v0 * frame, buf(o.in, o), (size_t)cn * frame,
                                                  hipMemcpyDeviceToDevice, s));
                    }
                    if (const char* e = launch_avgpool(h, buf(o.in, o), buf(o.out, o), cn, o.H * o.W, o.C, &dd, G, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                case OP_ENTRY_DROPOUT:
                    if (const char* e = launch_entry_dropout(h, pin_base, buf(o.out, o), o.in_elems, cn, &dd, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
                case OP_ENTRY_REDUCE:
                    if (const char* e = launch_entry_reduce(h, pin_base, o.skip_y ? nullptr : buf(o.out, o), LW(o.layer_a), LB(o.layer_a), buf(o.out2, o), o.C, o.Co2,
                                                            o.H * o.W, cn, &dd, s)) { h->err = e; return FAV_ERR_INVALID_ARG; }
                    break;
            }
            if (stage_here && o.kind != OP_AVGPOOL) {
                // the stage tap: the frames this op has written, to [virtual frame] of its buffer, behind the launch
                const size_t frame = (size_t)o.out_elems * 2;
                HIP_TRY(h, hipMemcpyAsync((char*)h->stage_tap.buf + (size_t)v0 * frame, buf(o.out, o), (size_t)cn * frame,
                                          hipMemcpyDeviceToDevice, s));
            }
        }
    }
    HIP_TRY(h, hipGetLastError());
    return FAV_OK;
}

void free_all(fav_handle* h) {
    for (auto& L : h->weights) {
        if (L.w_slab) (void)hipFree(L.w_slab);
        if (L.b_slab) (void)hipFree(L.b_slab);
        L.w_slab = L.b_slab = nullptr;
        L.w_m.clear(); L.b_m.clear();
    }
    for (int i = 0; i < 5; ++i) if (h->act[i]) (void)hipFree(h->act[i]);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->a1) (void)hipFree(h->a1);
    for (Lane& w : h->lanes) {
        if (w.stream) (void)hipStreamDestroy(w.stream);
        if (w.done) (void)hipEventDestroy(w.done);
    }
    if (h->ev_members) (void)hipEventDestroy(h->ev_members);
    for (auto& w_ : h->sk) if (w_.ws) { (void)hipFree(w_.ws); (void)hipFree(w_.flags); (void)hipFree(w_.err); }
    for (auto st_ : h->vit_streams) (void)hipStreamDestroy(st_);
    for (auto ev_ : h->vit_done) (void)hipEventDestroy(ev_);
    for (size_t i = 0; i + 1 < h->phase_out.size(); ++i) if (h->phase_out[i]) (void)hipFree(h->phase_out[i]);
    if (h->logits) (void)hipFree(h->logits);
    if (h->host_stage) (void)hipFree(h->host_stage);
    if (h->view_buf) (void)hipFree(h->view_buf);
    if (h->feat_buf) (void)hipFree(h->feat_buf);
    for (void* q : {(void*)h->ood.mu, (void*)h->ood.Pt, (void*)h->ood.Mt, (void*)h->ood.cls}) if (q) (void)hipFree(q);
    for (void* q : {h->knn.bank, h->knn.ws, (void*)h->knn.cls}) if (q) (void)hipFree(q);
    if (h->drift.ws) (void)hipFree(h->drift.ws);
    for (void* q : {h->patch.bank, h->patch.ws}) if (q) (void)hipFree(q);
    for (void* q : {h->map_tap.buf, h->stage_tap.buf, h->attn_tap.buf, h->curve.buf, h->rise.buf}) if (q) (void)hipFree(q);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    if (h->ev_last) (void)hipEventDestroy(h->ev_last);
    for (void* q : {h->v_patches, h->v_emb, h->v_x, h->v_y, h->v_qkv, h->v_hid, h->v_cls}) if (q) (void)hipFree(q);
    for (auto& e : h->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
}

// The attention tap's launch: the head-mean attention of n frames' qkv rows, to a [n][T][attn_ld(T)] (fav_rollout.hpp).  Booked in
// no kernel class and in no route report.  The arguments have been checked (attn_mean_dims_error, the pointers).
void launch_attn_mean(const void* qkv, float* a, int n, int T, int D, int heads, hipStream_t s) {
    const int nkt = (T + 15) / 16, groups = (nkt + ATTN_MEAN_WAVES - 1) / ATTN_MEAN_WAVES;
    void (*const fn)(const uint16_t*, float*, int, int, int, float) =
        nkt <= 2 ? attn_mean_kernel<2, false> : nkt == 13 ? attn_mean_kernel<13, true> : nkt == 16 ? attn_mean_kernel<16, true>
                                                                                          : attn_mean_kernel<16, false>;
    const size_t lds = (size_t)2 * nkt * 16 * 128;      // two K buffers: at most 64 KB
    hipLaunchKernelGGL(fn, dim3((unsigned)(n * groups)), dim3(64 * ATTN_MEAN_WAVES), lds, s, (const uint16_t*)qkv, a, T, D, heads,
                       (float)(1.0 / heads));
}

// One forward pass of the ViT encoder over n frames -> fp32 logits [n][cpad].
// Frames [f0, f0 + n) of the call's n_call: every buffer is indexed by frame, so two halves of a batch can run side by side
// on two streams (fav_classify_ex).
fav_status run_vit(fav_handle* h, const void* images_all, int layout, int f0, int n, int n_call, hipStream_t s) {
    const fav_config& c = h->cfg;
    const VitDef& V = kVit[c.arch - 2];
    const int ntok = h->plan.ntok, D = V.dim, gh = c.in_h / V.patch, gw = c.in_w / V.patch;
    const float inv_std[3] = {1.0f / c.stdev[0], 1.0f / c.stdev[1], 1.0f / c.stdev[2]};
    const size_t F = (size_t)f0, np = (size_t)gh * gw;
    const void* images = (const char*)images_all + F * c.in_h * c.in_w * 3 * (layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4);
    struct { void *v_patches, *v_emb, *v_x, *v_y, *v_qkv, *v_hid, *v_cls; float* logits; } B;
    B.v_patches = (char*)h->v_patches + F * np * (size_t)(V.patch * V.patch * 3) * 2;
    B.v_emb = (char*)h->v_emb + F * np * D * 2;
    B.v_x = (char*)h->v_x + F * ntok * D * 2;
    B.v_y = (char*)h->v_y + F * ntok * D * 2;
    B.v_qkv = (char*)h->v_qkv + F * ntok * 3 * D * 2;
    B.v_hid = (char*)h->v_hid + F * ntok * (size_t)V.mlp * 2;
    B.v_cls = (char*)h->v_cls + F * D * 2;
    B.logits = h->logits + F * h->plan.cpad;
    auto gemm = [&](int layer, const void* x, int rows_per_frame, const void* res, int act, void* y, int out_f32) -> const char* {
        const LayerShape& L = h->plan.layers[layer];
        const void* w = h->weights[layer].w_m[0];
        const float* bias = h->weights[layer].b_m[0];
        fav_conv_desc d;
        memset(&d, 0, sizeof d);
        d.x = x; d.w = w; d.bias = bias; d.res = res; d.y = y;
        d.n_frames = n; d.H = rows_per_frame; d.W = 1; d.Cin = L.k; d.Cout = L.cout;
        d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0; d.relu = act; d.out_f32 = out_f32; d.math_mode = c.math_mode;
        d.drop.site = -1;
        if (!out_f32 && c.math_mode == FAV_MATH_BF16 && L.cout == L.cout_pad &&
            launch_gemm_streamk(h, x, w, bias, res, y, (long long)n * rows_per_frame, L.k, L.cout, act, s)) return nullptr;
        return launch_conv(h, d, L.cout_pad, out_f32 ? L.cout_pad : L.cout, true, Group{}, s);
    };
#define FAV_VIT_TRY(expr)                                            \
    do {                                                             \
        if (const char* e_ = (expr)) { h->err = e_; return FAV_ERR_INVALID_ARG; } \
    } while (0)
    h->cur_op = -1;
    // patch embedding: normalise + im2col (k = (r*P + s)*3 + c), GEMM, add positions / class token
    FAV_VIT_TRY(launch_stem(h, images, layout, n, c.in_h, c.in_w, V.patch, V.patch, V.patch, 0, V.patch * V.patch * 3, c.mean, inv_std, B.v_patches, s));
    FAV_VIT_TRY(gemm(0, B.v_patches, gh * gw, nullptr, 0, B.v_emb, 0));
    launch_vit_assemble(h, B.v_emb, (const float*)h->weights[1].w_m[0], B.v_x, n, ntok, D, s);
    int li = 2;
    for (int blk = 0; blk < V.depth; ++blk, li += 6) {
        const LayerWeights &ln1 = h->weights[li], &ln2 = h->weights[li + 3];
        FAV_VIT_TRY(launch_layernorm(h, B.v_x, D, (const float*)ln1.w_m[0], ln1.b_m[0], B.v_y, (long long)n * ntok, D, 1e-6f, s));
        FAV_VIT_TRY(gemm(li + 1, B.v_y, ntok, nullptr, 0, B.v_qkv, 0));
        if (h->attn_tap.on)   // the attention tap: layer blk of this part's frames, at [blk][f0] of the call's n_call rows
            launch_attn_mean(B.v_qkv, (float*)h->attn_tap.buf + ((size_t)blk * n_call + F) * ntok * h->attn.ld, n, ntok, D, V.heads, s);
        FAV_VIT_TRY(launch_attention(h, B.v_qkv, B.v_y, n, ntok, D, V.heads, c.math_mode, s));
        FAV_VIT_TRY(gemm(li + 2, B.v_y, ntok, B.v_x, 0, B.v_x, 0));                 // x = x + proj(attn), in place tile by tile
        FAV_VIT_TRY(launch_layernorm(h, B.v_x, D, (const float*)ln2.w_m[0], ln2.b_m[0], B.v_y, (long long)n * ntok, D, 1e-6f, s));
        FAV_VIT_TRY(gemm(li + 4, B.v_y, ntok, nullptr, 2, B.v_hid, 0));              // GELU fused
        FAV_VIT_TRY(gemm(li + 5, B.v_hid, ntok, B.v_x, 0, B.v_x, 0));
    }
    const LayerWeights& lnf = h->weights[li];
    FAV_VIT_TRY(launch_layernorm(h, B.v_x, (long long)ntok * D, (const float*)lnf.w_m[0], lnf.b_m[0], B.v_cls, n, D, 1e-6f, s));   // class tokens only
    if (h->tap)   // the feature tap: this part's class tokens, in front of the fc launch
        HIP_TRY(h, hipMemcpyAsync((char*)h->feat_buf + F * D * 2, B.v_cls, (size_t)n * D * 2, hipMemcpyDeviceToDevice, s));
    FAV_VIT_TRY(gemm(li + 1, B.v_cls, 1, nullptr, 0, B.logits, 1));
#undef FAV_VIT_TRY
    return FAV_OK;
}

// The launch geometry of the kernels that work a frame in row groups (views_straight_kernel, occlude_kernel,
// rise_mask_kernel): G groups a row, `parts` blocks of 256 of them a frame, `blocks` over the `pairs` (frame, variant) pairs one
// launch covers, the grid they are spread over, and [lo, hi): the 4-byte aligned part of the n input frames
template <class U>
struct RowGroups { int parts; FastDiv div_g; long long blocks; dim3 grid; const U *lo, *hi; };
template <class U>
RowGroups<U> row_groups(const U* in, int n, int H, int W, long long pairs) {
    const int G = 1 + (W + 3) / 4;
    const int parts = (int)(((long long)H * G + 255) / 256);
    const long long blocks = pairs * parts, max_grid = (1ll << 24) - 1;
    const size_t units = (size_t)n * H * W * 3;
    return {parts, fastdiv_make((uint32_t)G), blocks, dim3((unsigned)std::min(blocks, max_grid)),
            (const U*)(((uintptr_t)in + 3) & ~(uintptr_t)3), (const U*)((uintptr_t)(in + units) & ~(uintptr_t)3)};
}
// a fill colour as the kernels take it: a uint8 frame's words hold one byte each
void fill_words(const uint32_t* fill, int layout, uint32_t out[3]) {
    for (int c = 0; c < 3; ++c) out[c] = layout == FAV_LAYOUT_NHWC_U8 ? (fill[c] & 255u) : fill[c];
}

// The two launches behind fav_op_views and a handle's views (fav_views.hpp): the views without transpose, those with.  The
// arguments have been checked (fav_check_views, the sizes, the alignment).
template <class U>
void launch_views_of(const U* in, U* out, int n, int H, int W, const fav_view* views, int n_views, hipStream_t s) {
    ViewsArg va;
    memset(&va, 0, sizeof va);
    memcpy(va.v, views, (size_t)n_views * sizeof(fav_view));
    const long long max_grid = (1ll << 24) - 1;
    for (int tr = 0; tr < 2; ++tr) {
        va.count = 0;
        for (int a = 0; a < n_views; ++a)
            if (views[a].transpose == tr) va.idx[va.count++] = (uint8_t)a;
        if (!va.count) continue;
        if (!tr) {
            const RowGroups<U> g = row_groups(in, n, H, W, (long long)va.count * n);
            hipLaunchKernelGGL((views_straight_kernel<U>), g.grid, dim3(256), 0, s, in, out, n, H, W, va, g.parts, g.div_g, g.blocks,
                               g.lo, g.hi);
        } else {
            const int t1 = (H + VW_TILE - 1) / VW_TILE;
            const long long tiles = (long long)va.count * n * t1 * t1;
            hipLaunchKernelGGL((views_transpose_kernel<U>), dim3((unsigned)std::min(tiles, max_grid)), dim3(256), 0, s, in, out, n, H,
                               va, t1, tiles);
        }
    }
}
void launch_views(const void* in, void* out, int n, int H, int W, int layout, const fav_view* views, int n_views, hipStream_t s) {
    if (layout == FAV_LAYOUT_NHWC_U8) launch_views_of((const uint8_t*)in, (uint8_t*)out, n, H, W, views, n_views, s);
    else launch_views_of((const uint32_t*)in, (uint32_t*)out, n, H, W, views, n_views, s);
}

// The launches behind the curve ops and fav_classify_curve (fav_curve.hpp).  The arguments have been checked.
void launch_rank_cells(const float* map, int n, int cells, int32_t* rank, hipStream_t s) {
    hipLaunchKernelGGL(rank_cells_kernel, dim3((unsigned)n), dim3(256), 0, s, map, cells, rank);
}
template <class U>
void launch_occlude_of(const U* in, U* out, const int32_t* rank, int n, int H, int W, const OccludeArg& oa, hipStream_t s) {
    const RowGroups<U> g = row_groups(in, n, H, W, n);
    hipLaunchKernelGGL((occlude_kernel<U>), g.grid, dim3(256), 0, s, in, out, rank, n, H, W, oa, g.parts, g.div_g, g.blocks, g.lo, g.hi);
}
void launch_occlude(const void* in, void* out, const int32_t* rank, int n, int H, int W, int layout, int mh, int mw, int mode, int S,
                    int s0, int s1, const uint32_t* fill, hipStream_t s) {
    OccludeArg oa;
    memset(&oa, 0, sizeof oa);
    fill_words(fill, layout, oa.fill);
    oa.mode = mode; oa.S = S; oa.s0 = s0; oa.s1 = s1; oa.mh = mh; oa.mw = mw; oa.cells = mh * mw;
    oa.wide = H > (1 << 23) || W > (1 << 23);
    oa.div_h = fastdiv_make((uint32_t)H); oa.div_w = fastdiv_make((uint32_t)W);
    if (layout == FAV_LAYOUT_NHWC_U8) launch_occlude_of((const uint8_t*)in, (uint8_t*)out, rank, n, H, W, oa, s);
    else launch_occlude_of((const uint32_t*)in, (uint32_t*)out, rank, n, H, W, oa, s);
}
// num_classes = 0: not known, only a negative class is out of range
void launch_curve(const float* prob, const int32_t* labels, const int32_t* classes, int n, int S, int cells, int mode, int num_classes,
                  float* curve, fav_curve_record* rec, hipStream_t s) {
    CurveParams cp;
    cp.prob = prob; cp.labels = labels; cp.classes = classes; cp.curve = curve; cp.rec = (int32_t*)rec;
    cp.n = n; cp.S = S; cp.cells = cells; cp.mode = mode; cp.num_classes = num_classes;
    cp.half_step = (float)(0.5 / S);
    hipLaunchKernelGGL(curve_kernel, dim3((unsigned)((n + CV_CURVE_THREADS - 1) / CV_CURVE_THREADS)), dim3(CV_CURVE_THREADS), 0, s, cp);
}

// The launches behind the RISE ops and fav_classify_rise (fav_rise.hpp).  The arguments have been checked.
template <class U>
void launch_rise_mask_of(const U* in, U* out, int n, int H, int W, const RiseArg& ra, const uint32_t* fill, int m0, int m1, hipStream_t s) {
    const RowGroups<U> g = row_groups(in, n, H, W, n);
    hipLaunchKernelGGL((rise_mask_kernel<U>), g.grid, dim3(256), 0, s, in, out, n, H, W, ra, fill[0], fill[1], fill[2], m0, m1, g.parts,
                       g.div_g, g.blocks, g.lo, g.hi);
}
void launch_rise_mask(const void* in, void* out, int n, int H, int W, int layout, const fav_rise& d, long long first_index, int m0, int m1,
                      hipStream_t s) {
    const RiseArg ra = rise_arg(d, first_index, H, W);
    uint32_t fill[3];
    fill_words(layout == FAV_LAYOUT_NHWC_U8 ? d.fill_u8 : d.fill_f32_bits, layout, fill);
    if (layout == FAV_LAYOUT_NHWC_U8) launch_rise_mask_of((const uint8_t*)in, (uint8_t*)out, n, H, W, ra, fill, m0, m1, s);
    else launch_rise_mask_of((const uint32_t*)in, (uint32_t*)out, n, H, W, ra, fill, m0, m1, s);
}
// num_classes = 0: not known, only a negative class is out of range
void launch_rise_accumulate(const float* prob, const int32_t* classes, int n, const fav_rise& d, long long first_index, int H, int W, int mh,
                            int mw, int num_classes, float* map, fav_rise_record* rec, hipStream_t s) {
    RiseAccParams p;
    p.prob = prob; p.classes = classes; p.map = map; p.rec = (int32_t*)rec;
    p.ra = rise_arg(d, first_index, H, W);
    p.n = n; p.N = d.n_masks; p.H = H; p.W = W; p.mh = mh; p.mw = mw; p.num_classes = num_classes;
    p.inv_n = (float)(1.0 / d.n_masks);
    hipLaunchKernelGGL(rise_accumulate_kernel, dim3((unsigned)n), dim3(RISE_ACC_THREADS), 0, s, p);
}

}  // namespace

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

int32_t fav_abi_version(void) { return FAV_ABI_VERSION; }

void fav_default_config(fav_config* c, int32_t arch) {
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->device = 0;
    c->arch = arch;
    c->num_classes = arch == FAV_ARCH_RESNET18_CIFAR ? 10 : 1000;
    c->in_h = c->in_w = (arch == FAV_ARCH_RESNET50 || arch == FAV_ARCH_VIT_B16) ? 224 : (arch == FAV_ARCH_VIT_TINY ? 64 : 32);
    c->max_batch = 256;
    c->mean[0] = 0.485f; c->mean[1] = 0.456f; c->mean[2] = 0.406f;
    c->stdev[0] = 0.229f; c->stdev[1] = 0.224f; c->stdev[2] = 0.225f;
    c->n_samples = 1;
    c->site_mask = 0;
    c->dropout_p = 0.f;
    c->seed = 0;
    c->temperature = 1.f;
    c->conf_kind = FAV_CONF_MAX_SOFTMAX;
    c->tau = 0.5f;
    c->math_mode = FAV_MATH_BF16;
    c->chunk_a = 0; c->chunk_b = 0; c->regroup_block = -1;
    c->n_members = 1;
}

const char* fav_last_error(const fav_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

fav_status fav_create(const fav_config* cfg, fav_handle** out) {
    if (out) *out = nullptr;
    if (!cfg || !out) { g_create_error = "fav_create: null argument"; return FAV_ERR_INVALID_ARG; }
    if (cfg->struct_size != sizeof(fav_config)) { g_create_error = "fav_create: fav_config.struct_size mismatch"; return FAV_ERR_INVALID_ARG; }
    if (cfg->arch < 0 || cfg->arch > 3) { g_create_error = "fav_create: unknown arch"; return FAV_ERR_UNSUPPORTED; }
    if (cfg->num_classes < 1 || cfg->num_classes > 1024 || cfg->max_batch < 1 || cfg->in_h < 8 || cfg->in_w < 8 ||
        cfg->n_samples < 1 || cfg->n_samples > 4096 || !(cfg->temperature > 0.f) || cfg->dropout_p < 0.f || cfg->dropout_p >= 1.f ||
        !(cfg->stdev[0] > 0.f && cfg->stdev[1] > 0.f && cfg->stdev[2] > 0.f) || cfg->math_mode < 0 || cfg->math_mode > 1 ||
        cfg->conf_kind < 0 || cfg->conf_kind > 2 || cfg->n_members < 0 || cfg->n_members > 64 ||
        cfg->tail_min_rows < -1 || cfg->ens_grouped_max < -1 || cfg->vit_streams < 0 || cfg->vit_streams > 4 || cfg->stem_fused < -1 || cfg->stem_fused > 0 ||
        (cfg->n_members > 1 && cfg->site_mask != 0 && cfg->dropout_p > 0.f)) {   // ensemble members are deterministic
        g_create_error = "fav_create: config value out of range";
        return FAV_ERR_INVALID_ARG;
    }
    if (std::lround((double)cfg->dropout_p * 256.0) > 255) {
        // the masks draw 8 bits and drop below round(256 p): 256 would drop every element and scale = 1 / (1 - 256/256) is infinite
        g_create_error = fmt("fav_create: dropout_p = %.9g rounds to the 8-bit threshold 256 (every element dropped, infinite scale); "
                             "the largest usable value is below 255.5 / 256", (double)cfg->dropout_p);
        return FAV_ERR_INVALID_ARG;
    }
    if (cfg->conf_kind == FAV_CONF_MUTUAL_INFO) {
        // the samples the head averages (the T_eff / n_members rule of plan_resnet; the ViT path is a single pass)
        const bool mc = !is_vit_arch(cfg->arch) && cfg->site_mask != 0 && std::lround((double)cfg->dropout_p * 256.0) > 0;
        const int T = cfg->n_members > 1 ? cfg->n_members : (mc ? cfg->n_samples : 1);
        if (T < 2 || cfg->num_classes < 2) {
            g_create_error = fmt("fav_create: conf_kind FAV_CONF_MUTUAL_INFO (mutual information) needs at least 2 samples "
                                 "(MC-Dropout with an active site, or n_members > 1) and 2 classes; this config has T=%d, "
                                 "num_classes=%d", T, cfg->num_classes);
            return FAV_ERR_INVALID_ARG;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        (void)hipGetLastError();
        g_create_error = fmt("fav_create: no usable HIP device (count=%d, requested=%d); this path has no CPU fallback", ndev, cfg->device);
        return FAV_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = fmt("fav_create: device %d is '%s', kernels are built for gfx950 only", cfg->device, prop.gcnArchName);
        return FAV_ERR_NO_DEVICE;
    }
    fav_handle* h = new fav_handle();
    h->cfg = *cfg;
    h->n_members = cfg->n_members > 1 ? cfg->n_members : 1;
    h->member_loaded.assign(h->n_members, 0);
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed"; delete h; return FAV_ERR_HIP; }
    h->vit = is_vit_arch(cfg->arch);
    fav_status st = h->vit ? plan_vit(h->cfg, &h->plan, &h->err) : plan_resnet(h->cfg, h->n_members, false, &h->plan, &h->err);
    if (st == FAV_OK) st = alloc_workspace(h);
    if (st != FAV_OK) { g_create_error = h->err; free_all(h); delete h; return st; }
    *out = h;
    return FAV_OK;
}

// The static schedule of a configuration as text, one line per op - no device needed (tests/test_host.py replays it
// symbolically and checks that the fused schedule computes the same dataflow as the layer-by-layer one).
//   "op <i> kind=<k> phase=<p> layer=<l> lc=<l> la=<l> in=<b> res=<b> out=<b> out2=<b> site=<s> relu=<r> suffix=<0|1>
//    rese=<0|1> skipy=<0|1> esite=<s>"
// buffers: 0..4 rotating, 5 im2col matrix, -1 frames, -2 phase input, -3 phase output, -4 none; suffix: the op's phase runs
// once per sample; rese / skipy: Op::res_entry / Op::skip_y; esite: the schedule's first dropout site (the entry op's).
fav_status fav_plan_schedule(const fav_config* cfg, int32_t flags, char* out, size_t cap) {
    if (!cfg || !out || cap < 2 || cfg->struct_size != sizeof(fav_config) || cfg->arch < 0 || cfg->arch > 1) return FAV_ERR_INVALID_ARG;
    Plan P;
    std::string err;
    fav_status st = plan_resnet(*cfg, cfg->n_members > 1 ? cfg->n_members : 1, (flags & 1) != 0, &P, &err);
    if (st != FAV_OK) { snprintf(out, cap, "%s", err.c_str()); return st; }
    std::string txt;
    for (size_t pi = 0; pi < P.phases.size(); ++pi)
        for (int i = P.phases[pi].op_begin; i < P.phases[pi].op_end; ++i) {
            const Op& o = P.ops[i];
            txt += fmt("op %d kind=%d phase=%zu layer=%d lc=%d la=%d in=%d res=%d out=%d out2=%d site=%d relu=%d suffix=%d rese=%d skipy=%d esite=%d\n", i, (int)o.kind, pi,
                       o.layer, o.layer_c, o.layer_a, o.in, o.res, o.out, o.out2, o.site, o.relu, (int)P.phases[pi].suffix, o.res_entry, o.skip_y, P.first_site);
        }
    if (txt.size() + 1 > cap) return FAV_ERR_INVALID_ARG;
    memcpy(out, txt.c_str(), txt.size() + 1);
    return FAV_OK;
}

void fav_destroy(fav_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    free_all(h);
    delete h;
}

fav_status fav_load_weights(fav_handle* h, const void* blob, size_t size) { return fav_load_member_weights(h, 0, blob, size); }

// Structural validation of a FAVW v1 blob; needs no device and no handle.  Every offset is taken from the
// (untrusted) file, so the range checks are written overflow-safe (off > size || bytes > size - off) and
// the data must be aligned for its element type (pack_blob emits 64-byte aligned offsets).
fav_status fav_check_blob(const void* blob, size_t size, char* err, size_t err_cap) {
    auto fail = [&](const std::string& m) {
        if (err && err_cap) { snprintf(err, err_cap, "%s", m.c_str()); }
        return FAV_ERR_BAD_BLOB;
    };
    if (err && err_cap) err[0] = 0;
    if (!blob || size < 32) return fail("blob too small");
    const uint8_t* p = (const uint8_t*)blob;
    uint32_t hdr[8];
    memcpy(hdr, p, 32);
    if (hdr[0] != 0x57564146u || hdr[1] != 1u) return fail("not a FAVW v1 blob");
    const size_t nl = hdr[4];
    if (nl == 0 || nl > 4096) return fail("implausible layer count");
    if ((size - 32) / 48 < nl) return fail("truncated layer table");
    const size_t data0 = 32 + 48 * nl;
    auto in_range = [&](uint64_t off, uint64_t bytes, uint64_t align) {
        return off >= data0 && off <= size && bytes <= size - off && off % align == 0;
    };
    for (size_t i = 0; i < nl; ++i) {
        uint32_t t[8];
        uint64_t off[2];
        memcpy(t, p + 32 + 48 * i, 32);
        memcpy(off, p + 32 + 48 * i + 32, 16);
        const uint64_t cout = t[0], cin = t[1], kh = t[2], kw = t[3];
        if (cout == 0 || cout > (1u << 24) || cin > (1u << 20) || kh > 64 || kw > 64) return fail(fmt("layer %zu: implausible shape", i));
        // every value must be finite: a NaN weight would defeat the pixel sanitiser and the bf16 rounding recipe (exponent all ones = Inf / NaN)
        auto f32_finite = [&](uint64_t o, uint64_t n) { for (uint64_t j = 0; j < n; ++j) { uint32_t u; memcpy(&u, p + o + 4 * j, 4); if ((u & 0x7F800000u) == 0x7F800000u) return false; } return true; };
        auto bf16_finite = [&](uint64_t o, uint64_t n) { for (uint64_t j = 0; j < n; ++j) { uint16_t u; memcpy(&u, p + o + 2 * j, 2); if ((u & 0x7F80u) == 0x7F80u) return false; } return true; };
        if (kh == 0) {   // a pair of fp32 vectors
            if (!in_range(off[0], cout * 4, 4) || !in_range(off[1], cout * 4, 4)) return fail(fmt("layer %zu data out of range", i));
            if (!f32_finite(off[0], cout) || !f32_finite(off[1], cout)) return fail(fmt("layer %zu holds a non-finite value", i));
            continue;
        }
        if (kw == 0 || cin == 0) return fail(fmt("layer %zu: implausible shape", i));
        const uint64_t k = kh * kw * cin;   // < 2^32
        if (k > (1ull << 32) / cout) return fail(fmt("layer %zu: implausible shape", i));
        if (!in_range(off[0], cout * k * 2, 2) || !in_range(off[1], cout * 4, 4)) return fail(fmt("layer %zu data out of range", i));
        if (!bf16_finite(off[0], cout * k) || !f32_finite(off[1], cout)) return fail(fmt("layer %zu holds a non-finite value", i));
    }
    return FAV_OK;
}

namespace {
// one allocation per layer for the weights of all members (and one for the biases): member m at slab + m * stride
fav_status alloc_layer_slabs(fav_handle* h, LayerWeights& L, size_t wbytes, size_t bbytes) {
    if (L.w_slab) return FAV_OK;
    L.w_stride = (wbytes + 255) / 256 * 256;
    L.b_stride = (bbytes + 255) / 256 * 256;
    HIP_TRY(h, hipMalloc(&L.w_slab, L.w_stride * h->n_members));
    HIP_TRY(h, hipMalloc(&L.b_slab, L.b_stride * h->n_members));
    L.w_m.assign(h->n_members, nullptr);
    L.b_m.assign(h->n_members, nullptr);
    for (int m = 0; m < h->n_members; ++m) {
        L.w_m[m] = (uint16_t*)((char*)L.w_slab + (size_t)m * L.w_stride);
        L.b_m[m] = (float*)((char*)L.b_slab + (size_t)m * L.b_stride);
    }
    return FAV_OK;
}
}  // namespace

fav_status fav_load_member_weights(fav_handle* h, int32_t member, const void* blob, size_t size) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (member < 0 || member >= h->n_members) { h->err = fmt("fav_load_member_weights: member %d outside [0, %d)", member, h->n_members); return FAV_ERR_INVALID_ARG; }
    {
        char msg[200];
        if (fav_check_blob(blob, size, msg, sizeof msg) != FAV_OK) { h->err = std::string("fav_load_weights: ") + msg; return FAV_ERR_BAD_BLOB; }
    }
    const uint8_t* p = (const uint8_t*)blob;
    uint32_t hdr[8];
    memcpy(hdr, p, 32);
    if ((int)hdr[2] != h->cfg.arch || (int)hdr[3] != h->cfg.num_classes || hdr[4] != h->plan.layers.size()) {
        h->err = fmt("fav_load_weights: blob is arch %u / %u classes / %u layers, handle expects %d / %d / %zu", hdr[2], hdr[3],
                     hdr[4], h->cfg.arch, h->cfg.num_classes, h->plan.layers.size());
        return FAV_ERR_BAD_BLOB;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::vector<uint16_t> wtmp;
    std::vector<float> btmp;
    for (size_t i = 0; i < h->plan.layers.size(); ++i) {
        const LayerShape& L = h->plan.layers[i];
        LayerWeights& Wt = h->weights[i];
        uint32_t t[8];
        uint64_t off[2];
        memcpy(t, p + 32 + 48 * i, 32);
        memcpy(off, p + 32 + 48 * i + 32, 16);
        if ((int)t[0] != L.cout || (int)t[1] != L.cin || (int)t[2] != L.kh || (int)t[3] != L.kw || (int)t[4] != L.stride ||
            (int)t[5] != L.pad) {
            h->err = fmt("fav_load_weights: layer %zu shape mismatch", i);
            return FAV_ERR_BAD_BLOB;
        }
        if (L.kh == 0) {   // a pair of fp32 vectors (LayerNorm gamma / beta, ViT position table)
            const size_t vb = (size_t)L.cout * 4;
            // (ranges and alignment already validated by fav_check_blob against these very table entries)
            if (fav_status st = alloc_layer_slabs(h, Wt, vb, vb)) return st;
            HIP_TRY(h, hipMemcpy(Wt.w_m[member], p + off[0], vb, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(Wt.b_m[member], p + off[1], vb, hipMemcpyHostToDevice));
            continue;
        }
        const size_t kreal = (size_t)L.kh * L.kw * L.cin;
        const size_t wbytes = (size_t)L.cout * kreal * 2, bbytes = (size_t)L.cout * 4;
        (void)wbytes;
        // device layout: [cout_pad][L.k] bf16, zero padded in both dimensions
        wtmp.assign((size_t)L.cout_pad * L.k, 0);
        const uint16_t* src = (const uint16_t*)(p + off[0]);
        for (int n = 0; n < L.cout; ++n) memcpy(&wtmp[(size_t)n * L.k], src + (size_t)n * kreal, kreal * 2);
        btmp.assign(L.cout_pad, 0.f);
        memcpy(btmp.data(), p + off[1], bbytes);
        if (fav_status st = alloc_layer_slabs(h, Wt, wtmp.size() * 2, btmp.size() * 4)) return st;
        HIP_TRY(h, hipMemcpy(Wt.w_m[member], wtmp.data(), wtmp.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(Wt.b_m[member], btmp.data(), btmp.size() * 4, hipMemcpyHostToDevice));
    }
    h->member_loaded[member] = 1;
    h->weights_loaded = true;
    for (char c : h->member_loaded) h->weights_loaded = h->weights_loaded && c;
    return FAV_OK;
}

namespace {
// orders this call's stream behind the previous user of the handle's buffers (see fav_handle::ev_last)
fav_status wait_last_use(fav_handle* h, hipStream_t s) {
    if (!h->ev_last) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming));
    if (h->ev_last_set) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_last, 0));
    return FAV_OK;
}
void mark_last_use(fav_handle* h, hipStream_t s) {
    if (h->ev_last && hipEventRecord(h->ev_last, s) == hipSuccess) h->ev_last_set = true;
}
// ---- the three ways a call's frames become logits; classify_on_stream picks one.  Inside a fork / join region nothing returns
//      (HIP_KEEP): a forked stream is always joined into the caller's.

// ViT: the batch in fav_config.vit_streams (default 2) parts on as many streams: at 197 rows per frame every GEMM of the encoder is a
// few hundred tiles, and the partial last round of one part's launch is filled by another part's (1: one stream)
fav_status run_vit_call(fav_handle* h, const Frames& f, hipStream_t s) {
    const int n = f.n;
    const int vit_streams = h->cfg.vit_streams <= 0 ? 2 : std::min(4, (int)h->cfg.vit_streams);
    if (!(vit_streams > 1 && n >= 8 * vit_streams)) {
        h->sk_slot = 0;
        return run_vit(h, f.images, f.layout, 0, n, n, s);
    }
    if (!h->ev_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    while ((int)h->vit_streams.size() < vit_streams) {
        hipStream_t st_; hipEvent_t ev_;
        HIP_TRY(h, hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        h->vit_streams.push_back(st_); h->vit_done.push_back(ev_);
    }
    HIP_TRY(h, hipEventRecord(h->ev_fork, s));
    fav_status st = FAV_OK;     // from here to the join nothing returns: a forked stream is always joined into s
    for (int part = 0; part < vit_streams; ++part) {
        const int f0 = (int)((long long)n * part / vit_streams), f1 = (int)((long long)n * (part + 1) / vit_streams);
        HIP_KEEP(h, st, hipStreamWaitEvent(h->vit_streams[part], h->ev_fork, 0));
        h->sk_slot = 1 + part;
        if (st == FAV_OK) st = run_vit(h, f.images, f.layout, f0, f1 - f0, n, h->vit_streams[part]);
        HIP_KEEP(h, st, hipEventRecord(h->vit_done[part], h->vit_streams[part]));
        HIP_KEEP(h, st, hipStreamWaitEvent(s, h->vit_done[part], 0));
    }
    return st;
}

// Every phase of `lane`, all (virtual) frames of the call
fav_status run_phases(fav_handle* h, const Frames& f, const Lane& lane) {
    for (size_t pi = 0; pi < h->plan.phases.size(); ++pi) {
        const long long dom = h->plan.phases[pi].suffix ? (long long)f.n * h->plan.T_eff : f.n;
        if (fav_status st = run_chunks(h, pi, f, lane, 0, dom)) return st;
    }
    return FAV_OK;
}

// An ensemble's small calls (will_group): every op ONE launch over all members (block row = member), on the caller's stream.
// At the 8-GPU share of configs[3] (32 frames) a member's launches are a few dozen tiles each; five of them in one grid fill
// the chip where five streams only interleave (profiles/r3aa_ens_grouped_ab.txt)
fav_status run_grouped(fav_handle* h, const Frames& f, hipStream_t s) {
    Lane lane = h->lanes[0];
    lane.stream = s;
    lane.groups = h->n_members;
    return run_phases(h, f, lane);
}

// Lanes side by side.  A single model is its one lane on the caller's stream: nothing to fork, nothing to join.  An ensemble
// forks from the caller's stream, one stream per member, and joins before the head.
fav_status run_lanes(fav_handle* h, const Frames& f, hipStream_t s) {
    if (h->lanes.size() == 1) {
        Lane lane = h->lanes[0];
        lane.stream = s;
        return run_phases(h, f, lane);
    }
    HIP_TRY(h, hipEventRecord(h->ev_members, s));
    fav_status st = FAV_OK;         // nothing returns between the fork and the join
    for (const Lane& w : h->lanes) HIP_KEEP(h, st, hipStreamWaitEvent(w.stream, h->ev_members, 0));
    // member by member.  (Enqueuing op by op ACROSS the members - so that all five streams start together and the launches
    // sharing the chip are the same op of different members - measured 5 % slower at 32 frames per call, 7 205 vs 7 585
    // frames/s, and 1 % slower at 256: profiles/r3j_ens_interleave_ab.txt.)
    for (const Lane& w : h->lanes)
        if (st == FAV_OK) st = run_phases(h, f, w);
    for (const Lane& w : h->lanes) {
        HIP_KEEP(h, st, hipEventRecord(w.done, w.stream));
        HIP_KEEP(h, st, hipStreamWaitEvent(s, w.done, 0));
    }
    return st;
}

// views: the frames are `views` views of f.n / views frames each, ordered [view][frame]; the head then averages views times as many
// samples on f.n / views frames (sample m * views + a: member or pass m under view a)
fav_status classify_on_stream(fav_handle* h, const Frames& f, const HeadOut& out, hipStream_t s, int views = 1) {
    h->ev_used = h->profiling ? h->ev_used : 0;
    fav_status st;
    if (h->vit) st = run_vit_call(h, f, s);
    else if (will_group(h->cfg, h->n_members, h->plan, f.n)) st = run_grouped(h, f, s);
    else st = run_lanes(h, f, s);
    if (st != FAV_OK) return st;
    const int T_head = (h->n_members > 1 ? h->n_members : h->plan.T_eff) * views, n_head = f.n / views;
    if (const char* e = launch_head(h, h->logits, T_head, n_head, h->cfg.num_classes, h->plan.cpad, h->cfg.temperature,
                                    h->cfg.conf_kind, h->cfg.tau, out, s)) {
        h->err = e;
        return FAV_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipGetLastError());
    h->last_T = T_head;
    h->last_n = n_head;
    if (h->tap) { h->feat_T = T_head; h->feat_n = n_head; }
    if (h->map_tap.on) { h->map_tap.S = h->map.S * views; h->map_tap.n = n_head; h->map_tap.views = h->n_views; }
    if (h->stage_tap.on) { h->stage_tap.S = h->stage.S * views; h->stage_tap.n = n_head; h->stage_tap.views = h->n_views; }
    if (h->attn_tap.on) { h->attn_tap.n = f.n; h->attn_tap.views = h->n_views; }
    return FAV_OK;
}

// The gate of every classify entry point: the argument checks, then classify_on_stream behind the previous user of the
// handle's buffers.  who: the public name the messages carry; bad: the entry point's own complaint about its buffers and
// parameters (NULL: none), reported after the handle and weights checks and before those on n, layout and first_index.
fav_status classify_gate(const char* who, fav_handle* h, const char* bad, const void* images, int32_t n, int32_t layout,
                         int64_t first_index, const HeadOut& out, void* stream) {
    route_clear();            // the report speaks of fav_op_* launches only: empty after a classify call, refused or not
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!h->weights_loaded) { h->err = fmt("%s: no weights loaded", who); return FAV_ERR_NO_WEIGHTS; }
    if (bad) { h->err = fmt("%s: %s", who, bad); return FAV_ERR_INVALID_ARG; }
    const int A = h->n_views;       // read once: this call's views
    if (A > 0 && (n < 1 || (long long)n * A > h->cfg.max_batch)) {
        h->err = fmt("%s: n=%d frames x n_views=%d views outside [1, max_batch=%d]", who, n, A, h->cfg.max_batch);
        return FAV_ERR_INVALID_ARG;
    }
    if (n < 1 || n > h->cfg.max_batch) { h->err = fmt("%s: n=%d outside [1, max_batch=%d]", who, n, h->cfg.max_batch); return FAV_ERR_INVALID_ARG; }
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) { h->err = fmt("%s: unknown layout", who); return FAV_ERR_INVALID_ARG; }
    if (first_index < 0 || first_index + n > 0xFFFFFFFFll) { h->err = fmt("%s: first_image_index out of range", who); return FAV_ERR_INVALID_ARG; }
    if (A > 0 && layout == FAV_LAYOUT_NHWC_F32 && ((uintptr_t)images & 3)) { h->err = fmt("%s: fp32 frames must be 4-byte aligned", who); return FAV_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (A > 0) {
        // the view buffer: max_batch frames of this call's layout.  Growing it (fp32 frames after uint8 ones) frees the old one,
        // which waits for the device
        const size_t need = (size_t)h->cfg.max_batch * h->cfg.in_h * h->cfg.in_w * 3 * (layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4);
        if (h->view_buf_bytes < need) {
            if (h->view_buf) { HIP_TRY(h, hipFree(h->view_buf)); h->view_buf = nullptr; h->view_buf_bytes = 0; }
            HIP_TRY(h, hipMalloc(&h->view_buf, need));
            h->view_buf_bytes = need;
        }
    }
    if (fav_status st = wait_last_use(h, s)) return st;
    fav_status st;
    if (A > 0) {
        launch_views(images, h->view_buf, n, h->cfg.in_h, h->cfg.in_w, layout, h->views, A, s);
        st = classify_on_stream(h, Frames{h->view_buf, layout, n * A, first_index}, out, s, A);
    } else {
        st = classify_on_stream(h, Frames{images, layout, n, first_index}, out, s);
    }
    route_clear();            // the report speaks of fav_op_* launches only
    mark_last_use(h, s);      // also after a failure: whatever was queued before it still uses the buffers
    return st;
}
const char* const kBadRecords = "null or misaligned buffer";
// why views and a perturbation head exclude each other, as fav_set_views and the head's setter both say it
const char* const kCurveViews = "an occluded frame's views are not what the map was made for";
const char* const kRiseViews = "a masked frame's views are not what the map is made for";
const char* bad_sets_args(const void* images, const HeadSets& hs) {
    if (const char* e = check_conformal(hs.cp)) return e;
    return !images || (!hs.rec && !hs.true_scores) || (hs.true_scores && !hs.true_labels) || ((uintptr_t)hs.rec & 7) ? kBadRecords : nullptr;
}
}  // namespace

fav_status fav_classify_ex(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                           int32_t* labels, float* conf, uint8_t* fail, float* score, void* stream) {
    HeadOut out;
    out.labels = labels; out.conf = conf; out.fail = fail; out.score = score;
    return classify_gate("fav_classify", h, !images || !labels || !conf ? "null buffer" : nullptr, images, n, layout, first_index, out,
                         stream);
}

fav_status fav_classify_records(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                                void* records, uint8_t* fail, float* score, void* stream) {
    HeadOut out;
    out.labels = (int32_t*)records; out.conf = (float*)records + 1; out.out_stride = 2; out.fail = fail; out.score = score;
    return classify_gate("fav_classify_records", h, !images || !records || ((uintptr_t)records & 7) ? kBadRecords : nullptr, images, n,
                         layout, first_index, out, stream);
}

fav_status fav_classify_uncertainty(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                                    fav_uncertainty* records, uint8_t* fail, float* score, void* stream) {
    static_assert(sizeof(fav_uncertainty) == 72, "fav_uncertainty is 18 dwords");
    HeadOut out;
    out.rec = records; out.fail = fail; out.score = score;
    return classify_gate("fav_classify_uncertainty", h, !images || !records || ((uintptr_t)records & 7) ? kBadRecords : nullptr, images,
                         n, layout, first_index, out, stream);
}

fav_status fav_classify_sets(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                             const fav_conformal* cp, fav_pred_set* records, uint8_t* fail, float* score, void* stream) {
    static_assert(sizeof(fav_pred_set) == 160, "fav_pred_set is 40 dwords");
    static_assert(sizeof(fav_conformal) == 32, "fav_conformal is 32 bytes");
    const HeadSets hs{cp, first_index, nullptr, nullptr, records};
    HeadOut out;
    out.sets = &hs; out.fail = fail; out.score = score;
    return classify_gate("fav_classify_sets", h, bad_sets_args(images, hs), images, n, layout, first_index, out, stream);
}

fav_status fav_conformal_scores(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                                const fav_conformal* cp, const int32_t* labels, float* scores, void* stream) {
    const HeadSets hs{cp, first_index, labels, scores, nullptr};
    HeadOut out;
    out.sets = &hs;
    return classify_gate("fav_conformal_scores", h, bad_sets_args(images, hs), images, n, layout, first_index, out, stream);
}

fav_status fav_classify_sweep(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                              const int32_t* true_labels, const float* temps, int32_t K, fav_calib_cell* cells, void* stream) {
    static_assert(sizeof(fav_calib_cell) == 16, "fav_calib_cell is 4 dwords");
    if (!h) return FAV_ERR_INVALID_ARG;
    const HeadSweep sw{temps, K, true_labels, cells};
    // the handle's conf_kind was checked against its sample count by fav_create
    const char* bad = check_sweep(sw, h->cfg.num_classes, -1, h->cfg.conf_kind);
    HeadOut out;
    out.sweep = &sw;
    return classify_gate("fav_classify_sweep", h, bad ? bad : (!images ? "null buffer" : nullptr), images, n, layout, first_index, out,
                         stream);
}

fav_status fav_set_temperature(fav_handle* h, float temperature) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!std::isfinite(temperature) || !(temperature > 0.f)) {
        h->err = fmt("fav_set_temperature: temperature %g is not finite and > 0", (double)temperature);
        return FAV_ERR_INVALID_ARG;
    }
    h->cfg.temperature = temperature;   // read on the host when a head is launched: enqueued calls carry their own copy
    return FAV_OK;
}

fav_status fav_set_tau(fav_handle* h, float tau) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (std::isnan(tau)) { h->err = "fav_set_tau: tau is NaN"; return FAV_ERR_INVALID_ARG; }
    h->cfg.tau = tau;
    return FAV_OK;
}

namespace {
// the samples the head averages on a handle with n_views views (0: off)
int head_samples(const fav_handle* h, int n_views) {
    return (h->n_members > 1 ? h->n_members : h->plan.T_eff) * std::max(1, n_views);
}
// what a host-only check (fav_check_views, fav_check_ood_model, fav_check_knn_bank) answers: `why` in err, "" and FAV_OK when fine
fav_status check_reply(const std::string& why, char* err, size_t cap) {
    if (err && cap) snprintf(err, cap, "%s", why.c_str());
    return why.empty() ? FAV_OK : FAV_ERR_INVALID_ARG;
}
}  // namespace

fav_status fav_check_views(const fav_view* views, int32_t n_views, int32_t H, int32_t W, char* err, size_t err_cap) {
    static_assert(sizeof(fav_view) == 24, "fav_view is 6 dwords");
    static_assert(FAV_MAX_VIEWS == VW_MAX_VIEWS && sizeof(ViewsArg) <= 2048, "the views travel in the kernel arguments");
    return check_reply(views_error(views, n_views, H, W), err, err_cap);
}

fav_status fav_set_views(fav_handle* h, const fav_view* views, int32_t n_views) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (n_views != 0) {
        char why[256];
        if (fav_check_views(views, n_views, h->cfg.in_h, h->cfg.in_w, why, sizeof why) != FAV_OK) {
            h->err = fmt("fav_set_views: %s", why);
            return FAV_ERR_INVALID_ARG;
        }
        const struct { bool on; const char *what, *why, *setter; } perturb[] = {{h->curve_on, "a curve", kCurveViews, "fav_set_curve"},
                                                                                {h->rise_on, "a RISE", kRiseViews, "fav_set_rise"}};
        for (const auto& p : perturb) {
            if (!p.on) continue;
            h->err = fmt("fav_set_views: %s descriptor is set; %s (clear it first: %s)", p.what, p.why, p.setter);
            return FAV_ERR_UNSUPPORTED;
        }
        if (!h->vit && h->plan.has_mc) {
            h->err = "fav_set_views: this handle draws MC-Dropout masks, which are keyed by batch row; views are not supported on it";
            return FAV_ERR_UNSUPPORTED;
        }
        // the view kernels hold a frame's work items in 32 bits (the limit fav_op_views states)
        if ((long long)h->cfg.in_h * h->cfg.in_w > 0x7FFFFFFFll / 12) {
            h->err = fmt("fav_set_views: in_h * in_w = %lld above (2^31 - 1) / 12 pixels", (long long)h->cfg.in_h * h->cfg.in_w);
            return FAV_ERR_INVALID_ARG;
        }
        if (n_views > h->cfg.max_batch) {
            h->err = fmt("fav_set_views: n_views=%d above max_batch=%d: not even one frame fits a call", n_views, h->cfg.max_batch);
            return FAV_ERR_INVALID_ARG;
        }
        if (head_samples(h, n_views) > 4096) {
            h->err = fmt("fav_set_views: %d members x %d views is above the heads' limit of 4096 samples", head_samples(h, 0), n_views);
            return FAV_ERR_INVALID_ARG;
        }
    }
    if (h->cfg.conf_kind == FAV_CONF_MUTUAL_INFO && head_samples(h, n_views) < 2) {
        h->err = fmt("fav_set_views: the confidence kind is FAV_CONF_MUTUAL_INFO and %d view(s) would leave it %d sample; change the "
                     "kind first (fav_set_conf_kind)", n_views, head_samples(h, n_views));
        return FAV_ERR_INVALID_ARG;
    }
    if (n_views) memcpy(h->views, views, (size_t)n_views * sizeof(fav_view));   // read on the host when a call is enqueued
    h->n_views = n_views;
    return FAV_OK;
}

fav_status fav_get_views(const fav_handle* h, fav_view* out, int32_t cap, int32_t* n_out) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (n_out) *n_out = h->n_views;
    if (out) for (int a = 0; a < cap && a < h->n_views; ++a) out[a] = h->views[a];
    return FAV_OK;
}

fav_status fav_set_conf_kind(fav_handle* h, int32_t conf_kind) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (conf_kind < 0 || conf_kind > 2) { h->err = fmt("fav_set_conf_kind: conf_kind=%d is not a fav_conf_kind", conf_kind); return FAV_ERR_INVALID_ARG; }
    if (conf_kind == FAV_CONF_MUTUAL_INFO && (head_samples(h, h->n_views) < 2 || h->cfg.num_classes < 2)) {
        h->err = fmt("fav_set_conf_kind: FAV_CONF_MUTUAL_INFO (mutual information) needs at least 2 samples and 2 classes; this handle "
                     "has T=%d (views included), num_classes=%d", head_samples(h, h->n_views), h->cfg.num_classes);
        return FAV_ERR_INVALID_ARG;
    }
    h->cfg.conf_kind = conf_kind;   // read on the host when a head is launched
    return FAV_OK;
}

fav_status fav_classify(fav_handle* h, const void* images, int32_t n, int32_t layout, int32_t* labels, float* conf,
                        void* stream) {
    return fav_classify_ex(h, images, n, layout, 0, labels, conf, nullptr, nullptr, stream);
}

fav_status fav_classify_host(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index,
                             int32_t* labels, float* conf, uint8_t* fail, float* score) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!images || !labels || !conf || n < 1 || n > h->cfg.max_batch) { h->err = "fav_classify_host: bad argument"; return FAV_ERR_INVALID_ARG; }
    // validate everything that sizes the copy BEFORE touching the caller's buffer
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) { h->err = "fav_classify_host: unknown layout"; return FAV_ERR_INVALID_ARG; }
    if (!h->weights_loaded) { h->err = "fav_classify_host: no weights loaded"; return FAV_ERR_NO_WEIGHTS; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->host_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
    hipStream_t hs = h->host_stream;
    const size_t bpe = layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4;
    const size_t img_bytes = (size_t)h->cfg.max_batch * h->cfg.in_h * h->cfg.in_w * 3 * 4;
    const size_t res_off = (img_bytes + 255) / 256 * 256;
    if (!h->host_stage) HIP_TRY(h, hipMalloc(&h->host_stage, res_off + (size_t)h->cfg.max_batch * 16 + 256));
    char* base = (char*)h->host_stage;
    int32_t* dl = (int32_t*)(base + res_off);
    float* dc = (float*)(dl + h->cfg.max_batch);
    float* ds = dc + h->cfg.max_batch;
    uint8_t* df = (uint8_t*)(ds + h->cfg.max_batch);
    // everything on the handle's own stream; only that stream is synchronised (not the device)
    HIP_TRY(h, hipMemcpyAsync(base, images, (size_t)n * h->cfg.in_h * h->cfg.in_w * 3 * bpe, hipMemcpyHostToDevice, hs));
    fav_status st = fav_classify_ex(h, base, n, layout, first_index, dl, dc, df, ds, hs);
    if (st != FAV_OK) return st;
    HIP_TRY(h, hipMemcpyAsync(labels, dl, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
    HIP_TRY(h, hipMemcpyAsync(conf, dc, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
    if (score) HIP_TRY(h, hipMemcpyAsync(score, ds, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
    if (fail) HIP_TRY(h, hipMemcpyAsync(fail, df, (size_t)n, hipMemcpyDeviceToHost, hs));
    HIP_TRY(h, hipStreamSynchronize(hs));
    return FAV_OK;
}

fav_status fav_get_logits(fav_handle* h, float* out, int32_t* t_out, int32_t* n_out, void* stream) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (h->last_n == 0) { h->err = "fav_get_logits: no classify call yet"; return FAV_ERR_INVALID_ARG; }
    if (t_out) *t_out = h->last_T;
    if (n_out) *n_out = h->last_n;
    if (out) {
        if (fav_status st = wait_last_use(h, (hipStream_t)stream)) return st;
        HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)h->cfg.num_classes * 4, h->logits, (size_t)h->plan.cpad * 4,
                                    (size_t)h->cfg.num_classes * 4, (size_t)h->last_T * h->last_n,
                                    hipMemcpyDeviceToDevice, (hipStream_t)stream));
        mark_last_use(h, (hipStream_t)stream);
    }
    return FAV_OK;
}

// ---- feature tap and OOD scoring (fav_ood.hpp) ------------------------------
namespace {
// the width of the row the final fc reads
int feature_width(const fav_handle* h) { return h->vit ? kVit[h->cfg.arch - 2].dim : h->plan.ops.back().C; }

// The scoring head: one launch, x and g in LDS.  The arguments have been checked (ood_dims_error, the pointers).
void launch_ood(const void* feat, int S, int n, int D, int k, int R, const float* mu, const float* Pt, const float* Mt,
                const int32_t* cls, const int32_t* labels, float threshold, fav_ood_record* rec, hipStream_t s) {
    OodParams p;
    p.feat = (const uint16_t*)feat; p.mu = mu; p.Pt = Pt; p.Mt = Mt; p.cls = cls; p.labels = labels; p.rec = (int32_t*)rec;
    p.S = S; p.n = n; p.D = D; p.k = k; p.R = R;
    p.inv_S = (float)(1.0 / S); p.threshold = threshold;
    const int fpb = ood_frames_per_block(n, D, k);
    const size_t lds = (size_t)fpb * (size_t)(D + k) * 4;
    const dim3 grid((unsigned)((n + fpb - 1) / fpb));
    if (fpb == 4) hipLaunchKernelGGL(ood_score_kernel<4>, grid, dim3(OOD_THREADS), lds, s, p);
    else if (fpb == 2) hipLaunchKernelGGL(ood_score_kernel<2>, grid, dim3(OOD_THREADS), lds, s, p);
    else hipLaunchKernelGGL(ood_score_kernel<1>, grid, dim3(OOD_THREADS), lds, s, p);
}

void free_ood(fav_handle::OodDev* o) {
    for (void* q : {(void*)o->mu, (void*)o->Pt, (void*)o->Mt, (void*)o->cls}) if (q) (void)hipFree(q);
    *o = fav_handle::OodDev{};
}
// the host waits for what has been enqueued on the handle (its last call's event)
fav_status wait_enqueued(fav_handle* h) {
    if (h->ev_last_set) HIP_TRY(h, hipEventSynchronize(h->ev_last));
    return FAV_OK;
}
// The tap is on iff the caller asked for it or a head reads it.  tap_sync brings the handle in line with `on`: tap_wanted
// once one of the four facts has changed, or true in front of a fact that is about to (only that can fail, and then nothing
// has changed).  Every transition forgets the last call's sizes: fav_get_features has nothing until the next call.
bool tap_wanted(const fav_handle* h) { return h->tap_user || h->ood_on || h->knn_on || h->drift_on; }
fav_status tap_sync(fav_handle* h, bool on) {
    if (on && !h->feat_buf) {
        const int D = feature_width(h);
        const size_t rows = (size_t)(h->n_members > 1 ? h->n_members : h->plan.T_eff) * h->cfg.max_batch;
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        HIP_TRY(h, hipMalloc(&h->feat_buf, rows * D * 2 + 256));
        h->feat_D = D;
    }
    if (on != h->tap) { h->tap = on; h->feat_T = h->feat_n = 0; }
    return FAV_OK;
}

// ---- the frames the three feature heads share (fav_set_ood / fav_set_knn / fav_set_drift and their fav_classify_*)
// the members of a deep ensemble have a feature space each: `what` ("an OOD model", "a k-NN bank", ..) is refused on one
fav_status refuse_ensemble(fav_handle* h, const char* fn, const char* what) {
    if (h->n_members <= 1) return FAV_OK;
    h->err = fmt("%s: the members of a deep ensemble do not share a feature space; %s is not supported on it", fn, what);
    return FAV_ERR_UNSUPPORTED;
}
extern "C++" {   // templates
// a setter's NULL argument: the head `cur` goes, and with the last reader the tap
template <class Dev>
fav_status head_clear(fav_handle* h, Dev& cur, bool& on, void (*free_dev)(Dev*)) {
    if (!on) return FAV_OK;
    if (fav_status st = wait_enqueued(h)) return st;
    free_dev(&cur);
    on = false;
    return tap_sync(h, tap_wanted(h));
}
// ... and its last step: `fresh`, the device copy it built (`built`; false: it failed and has written h->err), becomes the
// head.  Any failure frees `fresh` and leaves the handle, the tap included, as it was.
template <class Dev>
fav_status head_commit(fav_handle* h, Dev& cur, bool& on, Dev& fresh, void (*free_dev)(Dev*), bool built) {
    fav_status st = built ? tap_sync(h, true) : FAV_ERR_HIP;
    if (st == FAV_OK && on) st = wait_enqueued(h);
    if (st != FAV_OK) {
        free_dev(&fresh);
        (void)tap_sync(h, tap_wanted(h));
        return st;
    }
    if (on) free_dev(&cur);
    cur = fresh;
    on = true;
    return FAV_OK;
}

// A classify call with a feature head behind it: fav_classify_ex, then `launch(stream)` on the same stream, which reads the
// tap (feat_T x feat_n are this call's samples and frames) and returns its launcher's refusal, if it has one.  `on`: the
// head's flag; `what` and `setter` name what is missing when it is off.
template <class Launch>
fav_status classify_feature_head(fav_handle* h, bool fav_handle::*on, const char* fn, const char* what, const char* setter,
                                 const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels, float* conf,
                                 uint8_t* fail, float* score, const void* records, void* stream, Launch launch) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!(h->*on)) { route_clear(); h->err = fmt("%s: no %s set (%s)", fn, what, setter); return FAV_ERR_INVALID_ARG; }
    if (!records || ((uintptr_t)records & 7)) { route_clear(); h->err = fmt("%s: %s", fn, kBadRecords); return FAV_ERR_INVALID_ARG; }
    if (fav_status st = fav_classify_ex(h, images, n, layout, first_index, labels, conf, fail, score, stream)) return st;
    hipStream_t s = (hipStream_t)stream;
    const char* e = launch(s);
    route_clear();            // the report speaks of fav_op_* launches only
    mark_last_use(h, s);
    if (e) { h->err = fmt("%s: %s", fn, e); return FAV_ERR_INVALID_ARG; }
    HIP_TRY(h, hipGetLastError());
    return FAV_OK;
}

// ---- the steps the two localisation taps and their heads share (fav_handle::LocTap: the map tap with fav_cam and
//      fav_classify_cam, the attention tap with fav_rollout and fav_classify_rollout).  The nouns of a tap in its refusals:
struct TapWords { const char *tap, *setter, *getter, *thing; };
const TapWords kMapWords = {"map", "fav_set_map_tap", "fav_get_maps", "map"};
const TapWords kStageWords = {"stage", "fav_set_stage_tap", "fav_get_stage_maps", "map"};
const TapWords kAttnWords = {"attention", "fav_set_attn_tap", "fav_get_attention", "rollout"};
// sizes for the caller: each pointer may be NULL
using Sizes = std::initializer_list<std::pair<int32_t*, int>>;
void put_sizes(Sizes sizes) { for (const auto& s : sizes) if (s.first) *s.first = s.second; }
// A fav_*_tap_info: the config checks, then `fill(&why)` plans the configuration and writes the sizes; the reply goes into err.
// unsupported: the tap's refusals from the config alone; samples: n_samples counts (the maps are one a sample)
template <class Fill>
fav_status tap_info(const char* fn, const fav_config* cfg, const char* (*unsupported)(int, int, int), bool samples, char* err,
                    size_t err_cap, Fill fill) {
    auto reply = [&](fav_status st, const char* why) {
        if (err && err_cap) snprintf(err, err_cap, "%s", st ? fmt("%s: %s", fn, why).c_str() : "");
        return st;
    };
    if (!cfg || cfg->struct_size != sizeof(fav_config)) return reply(FAV_ERR_INVALID_ARG, "null config or struct_size mismatch");
    if (cfg->arch < 0 || cfg->arch > 3) return reply(FAV_ERR_UNSUPPORTED, "unknown arch");
    if (const char* why = unsupported(cfg->arch, cfg->n_members, cfg->math_mode)) return reply(FAV_ERR_UNSUPPORTED, why);
    if (cfg->max_batch < 1 || (samples && (cfg->n_samples < 1 || cfg->n_samples > 4096)) || cfg->in_h < 8 || cfg->in_w < 8 || cfg->num_classes < 1)
        return reply(FAV_ERR_INVALID_ARG, "config value out of range");
    std::string why;
    const fav_status st = fill(&why);
    return reply(st, why.c_str());
}
// The tap goes off: the flag and the last call's counts first, then the wait for what is enqueued, then the buffer
fav_status tap_off(fav_handle* h, fav_handle::LocTap& t) {
    if (!t.on) return FAV_OK;
    t.on = false;
    t.S = t.n = t.views = 0;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (fav_status st = wait_enqueued(h)) return st;
    void* buf = t.buf;
    t.buf = nullptr;
    if (buf) HIP_TRY(h, hipFree(buf));
    return FAV_OK;
}
// The tap goes on (a tap that is on stays as it is, once the checks have passed).  unsupported: the tap's refusal of this
// handle, if any; `make_dims()`: what the tap holds (only a supported handle has any), kept in `dims`; what: tap_budget_error's
template <class Dims, class MakeDims>
fav_status tap_on(fav_handle* h, const char* fn, fav_handle::LocTap& t, Dims& dims, const char* unsupported, const char* what,
                  size_t max_bytes, size_t default_budget, MakeDims make_dims) {
    if (unsupported) { h->err = fmt("%s: %s", fn, unsupported); return FAV_ERR_UNSUPPORTED; }
    const Dims d = make_dims();
    const std::string why = tap_budget_error(what, d.bytes, max_bytes, default_budget);
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (t.on) return FAV_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMalloc(&t.buf, d.bytes + 256));
    dims = d;
    t.S = t.n = t.views = 0;
    t.on = true;
    return FAV_OK;
}
// What the last call left in the tap: its sizes, and with `out` the first `bytes` of the buffer, behind the buffer's last use
fav_status tap_get(fav_handle* h, const char* fn, const TapWords& w, const fav_handle::LocTap& t, Sizes sizes, void* out, size_t bytes,
                   void* stream) {
    if (!t.on) { h->err = fmt("%s: the %s tap is off (%s)", fn, w.tap, w.setter); return FAV_ERR_INVALID_ARG; }
    if (t.n == 0) { h->err = fmt("%s: no classify call since the tap was turned on", fn); return FAV_ERR_INVALID_ARG; }
    put_sizes(sizes);
    if (out) {
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        if (fav_status st = wait_last_use(h, s)) return st;
        HIP_TRY(h, hipMemcpyAsync(out, t.buf, bytes, hipMemcpyDeviceToDevice, s));
        mark_last_use(h, s);
    }
    return FAV_OK;
}
// What a head's two entry points refuse alike about the handle's state, before anything is enqueued (FAV_OK: nothing).
// bad_buffers: an output is null or misaligned; `dims_error()`: the head's own ranges, asked only once the tap is known to be on
template <class DimsError>
fav_status map_head_gate(fav_handle* h, const char* fn, const TapWords& w, const fav_handle::LocTap& t, bool bad_buffers, DimsError dims_error) {
    if (!t.on) { h->err = fmt("%s: the %s tap is off (%s)", fn, w.tap, w.setter); return FAV_ERR_INVALID_ARG; }
    if (h->n_views > 0) {
        h->err = fmt("%s: views are set; a view's %s lies in that view's frame and averaging them mis-registers (%s still works)", fn, w.thing, w.getter);
        return FAV_ERR_UNSUPPORTED;
    }
    if (bad_buffers) { h->err = fmt("%s: %s", fn, kBadRecords); return FAV_ERR_INVALID_ARG; }
    const std::string why = dims_error();
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    return FAV_OK;
}
// the head's `launch(stream)` on what the tap holds (its launcher's refusal, or nullptr), booked as the buffers' last use
template <class Launch>
fav_status map_head_on_stream(fav_handle* h, const char* fn, Launch launch, hipStream_t s) {
    const char* e = launch(s);
    route_clear();            // the report speaks of fav_op_* launches only
    mark_last_use(h, s);
    if (e) { h->err = fmt("%s: %s", fn, e); return FAV_ERR_HIP; }
    HIP_TRY(h, hipGetLastError());
    return FAV_OK;
}
// fav_cam, fav_rollout: the head on what the LAST call left in the tap, behind whatever used the handle's buffers last
template <class DimsError, class Launch>
fav_status map_head_on_last_call(fav_handle* h, const char* fn, const TapWords& w, fav_handle::LocTap fav_handle::*tap, bool bad_buffers,
                                 DimsError dims_error, void* stream, Launch launch) {
    route_clear();
    if (!h) return FAV_ERR_INVALID_ARG;
    const fav_handle::LocTap& t = h->*tap;
    if (fav_status st = map_head_gate(h, fn, w, t, bad_buffers, dims_error)) return st;
    if (t.n == 0) { h->err = fmt("%s: no classify call since the tap was turned on", fn); return FAV_ERR_INVALID_ARG; }
    if (t.views > 0) { h->err = fmt("%s: the last call ran under views; their %ss lie in each view's own frame", fn, w.thing); return FAV_ERR_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (fav_status st = wait_last_use(h, s)) return st;
    return map_head_on_stream(h, fn, launch, s);
}
// fav_classify_cam, fav_classify_rollout: fav_classify_ex, then the head on the same stream
template <class DimsError, class Launch>
fav_status classify_map_head(fav_handle* h, const char* fn, const TapWords& w, fav_handle::LocTap fav_handle::*tap, bool bad_buffers,
                             DimsError dims_error, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                             float* conf, uint8_t* fail, float* score, void* stream, Launch launch) {
    route_clear();
    if (!h) return FAV_ERR_INVALID_ARG;
    if (fav_status st = map_head_gate(h, fn, w, h->*tap, bad_buffers, dims_error)) return st;
    if (fav_status st = fav_classify_ex(h, images, n, layout, first_index, labels, conf, fail, score, stream)) return st;
    return map_head_on_stream(h, fn, launch, (hipStream_t)stream);
}

// ---- the steps the two perturbation heads share (fav_set_curve / fav_set_rise and their fav_classify_*): each perturbs the
// frames, classifies every perturbed copy and reduces one class's probability over the copies
// a setter's NULL argument: the head goes with its buffer, once what is enqueued has run
fav_status perturb_clear(fav_handle* h, fav_handle::PerturbDev& cur, bool& on) {
    if (!on) return FAV_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (fav_status st = wait_enqueued(h)) return st;
    on = false;
    void* buf = cur.buf;
    cur = fav_handle::PerturbDev{};
    if (buf) HIP_TRY(h, hipFree(buf));
    return FAV_OK;
}
// ... and a descriptor: `check(layout)` is the descriptor's complaint, asked under both layouts; `views_why` the head's
// sentence when views are set; then `plan(fresh, what)` names the parts of the buffer - bytes each, where its address goes -
// and says in `what` whose they are, for the reply when ONE allocation with every part on a 256-byte boundary fails.  A
// buffer being replaced is freed once what is enqueued, which still uses it, has run.  Any failure leaves the handle as it was.
struct PerturbPart { size_t bytes; void** at; };
template <class Check, class Plan>
fav_status perturb_commit(fav_handle* h, const char* fn, fav_handle::PerturbDev& cur, bool& on, Check check, const char* views_why, Plan plan) {
    std::string why = check(FAV_LAYOUT_NHWC_U8);
    if (why.empty()) why = check(FAV_LAYOUT_NHWC_F32);
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (h->n_views > 0) { h->err = fmt("%s: views are set; %s (turn them off first: fav_set_views)", fn, views_why); return FAV_ERR_UNSUPPORTED; }
    fav_handle::PerturbDev fresh;
    std::string what;
    const std::vector<PerturbPart> parts = plan(fresh, what);
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t bytes = 0;
    for (const PerturbPart& p : parts) bytes += pad(p.bytes);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (hipMalloc(&fresh.buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->err = fmt("%s: cannot allocate the %zu bytes %s takes", fn, bytes, what.c_str());
        return FAV_ERR_HIP;
    }
    char* q = (char*)fresh.buf;
    for (const PerturbPart& p : parts) { *p.at = q; q += pad(p.bytes); }
    if (on) {
        if (fav_status st = wait_enqueued(h)) { (void)hipFree(fresh.buf); return st; }
        if (cur.buf) (void)hipFree(cur.buf);
    }
    cur = fresh;
    on = true;
    return FAV_OK;
}
// the parts both heads have: the perturbed frames of one pass, `passes` probability planes, the unperturbed pass's label and
// confidence, for the handle's max_batch frames; d.passes is set here
std::vector<PerturbPart> perturb_parts(const fav_handle* h, fav_handle::PerturbDev& d, int passes) {
    const size_t B = (size_t)h->cfg.max_batch;
    d.passes = passes;
    return {{B * h->cfg.in_h * h->cfg.in_w * 3 * 4, &d.frames}, {(size_t)passes * B * 4, (void**)&d.prob}, {B * 4, (void**)&d.lab0},
            {B * 4, (void**)&d.conf0}};
}
// One pass of a perturbation head: the frames to classify, and the planes the class probability and (curve) the label go to
struct PerturbPass { const void* frames; float* prob; int32_t* lab; };
// fav_classify_curve, fav_classify_rise: the argument gate - `missing` names what is not set when `on` is off, `own()` is
// the head's complaint about its map and mode - then, behind the previous user of the handle's buffers, the passes.
// `pass(k, s)` enqueues the perturbation of pass k and says what to classify and where to; pass 0, the unperturbed one, also
// writes the caller's labels / conf or the handle's own copies, and a second head launch on its logits fills its plane.
// `reduce(classes, s)` enqueues the head's reduction over the planes; classes: the caller's, or pass 0's labels.
template <class Own, class Pass, class Reduce>
fav_status classify_perturb_head(fav_handle* h, const char* fn, bool fav_handle::*on, const char* missing,
                                 fav_handle::PerturbDev fav_handle::*dev, bool bad_buffers, const void* images, int32_t n, int32_t layout,
                                 int64_t first_index, const int32_t* classes, int32_t* labels, float* conf, void* stream, Own own, Pass pass,
                                 Reduce reduce) {
    route_clear();
    if (!h) return FAV_ERR_INVALID_ARG;
    auto refuse = [&](const std::string& why) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; };
    if (!h->weights_loaded) { h->err = fmt("%s: no weights loaded", fn); return FAV_ERR_NO_WEIGHTS; }
    if (!(h->*on)) return refuse(missing);
    if (bad_buffers) return refuse(kBadRecords);
    if (n < 1 || n > h->cfg.max_batch) return refuse(fmt("n=%d outside [1, max_batch=%d]", n, h->cfg.max_batch));
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return refuse("unknown layout");
    if (layout == FAV_LAYOUT_NHWC_F32 && ((uintptr_t)images & 3)) return refuse("fp32 frames must be 4-byte aligned");
    if (first_index < 0 || first_index + n > 0xFFFFFFFFll) return refuse("first_image_index out of range");
    const std::string why = own();
    if (!why.empty()) return refuse(why);
    if (h->n_views > 0) { h->err = fmt("%s: views are set", fn); return FAV_ERR_UNSUPPORTED; }   // fav_set_views refuses them; kept as a guard
    const fav_handle::PerturbDev& d = h->*dev;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (fav_status st = wait_last_use(h, s)) return st;
    int32_t* const lab0 = labels ? labels : d.lab0;
    const int32_t* const cls = classes ? classes : lab0;
    fav_status st = FAV_OK;
    for (int k = 0; k < d.passes && st == FAV_OK; ++k) {
        const PerturbPass p = pass(k, s);
        const Frames f{p.frames, layout, n, first_index};
        const HeadClassProb cp{cls, p.prob, p.lab};
        HeadOut out;
        if (k > 0) {
            out.cprob = &cp;
            st = classify_on_stream(h, f, out, s);
            continue;
        }
        out.labels = lab0; out.conf = conf ? conf : d.conf0;
        st = classify_on_stream(h, f, out, s);
        if (st != FAV_OK) break;
        HeadOut second;
        second.cprob = &cp;
        if (const char* e = launch_head(h, h->logits, h->last_T, n, h->cfg.num_classes, h->plan.cpad, h->cfg.temperature, h->cfg.conf_kind,
                                        h->cfg.tau, second, s)) {
            h->err = fmt("%s: %s", fn, e);
            st = FAV_ERR_INVALID_ARG;
        }
    }
    if (st == FAV_OK) reduce(cls, s);
    route_clear();            // the report speaks of fav_op_* launches only
    mark_last_use(h, s);      // also after a failure: whatever was queued before it still uses the buffers
    if (st != FAV_OK) return st;
    HIP_TRY(h, hipGetLastError());
    return FAV_OK;
}
}  // extern "C++"
}  // namespace

fav_status fav_set_feature_tap(fav_handle* h, int32_t enable) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (enable) {
        if (fav_status st = tap_sync(h, true)) return st;
        h->tap_user = true;     // the caller's own tap outlives a model and a bank
        return FAV_OK;
    }
    if (h->ood_on) { h->err = "fav_set_feature_tap: an OOD model is set, which reads the tap; clear it first (fav_set_ood)"; return FAV_ERR_INVALID_ARG; }
    if (h->knn_on) { h->err = "fav_set_feature_tap: a k-NN bank is set, which reads the tap; clear it first (fav_set_knn)"; return FAV_ERR_INVALID_ARG; }
    if (h->drift_on) { h->err = "fav_set_feature_tap: a drift reference is set, which reads the tap; clear it first (fav_set_drift)"; return FAV_ERR_INVALID_ARG; }
    h->tap_user = false;
    return tap_sync(h, false);
}

fav_status fav_get_features(fav_handle* h, float* out, int32_t* s_out, int32_t* n_out, int32_t* d_out, void* stream) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!h->tap) { h->err = "fav_get_features: the feature tap is off (fav_set_feature_tap)"; return FAV_ERR_INVALID_ARG; }
    if (h->feat_n == 0) { h->err = "fav_get_features: no classify call since the tap was turned on"; return FAV_ERR_INVALID_ARG; }
    if ((uintptr_t)out & 15) { h->err = "fav_get_features: out_dev must be 16-byte aligned"; return FAV_ERR_INVALID_ARG; }
    if (s_out) *s_out = h->feat_T;
    if (n_out) *n_out = h->feat_n;
    if (d_out) *d_out = h->feat_D;
    if (out) {
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        if (fav_status st = wait_last_use(h, s)) return st;
        const long long groups = (long long)h->feat_T * h->feat_n * h->feat_D / 8;
        hipLaunchKernelGGL(features_to_f32_kernel, dim3(grid_for(groups)), dim3(256), 0, s, (const uint4*)h->feat_buf, (float4*)out, groups);
        HIP_TRY(h, hipGetLastError());
        mark_last_use(h, s);
    }
    return FAV_OK;
}

fav_status fav_check_ood_model(const fav_ood_model* m, int32_t D_expected, char* err, size_t err_cap) {
    static_assert(sizeof(fav_ood_record) == 16, "fav_ood_record is 4 dwords");
    return check_reply(ood_model_error(m, D_expected), err, err_cap);
}

fav_status fav_set_ood(fav_handle* h, const fav_ood_model* m) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!m) return head_clear(h, h->ood, h->ood_on, free_ood);
    const std::string why = ood_model_error(m, feature_width(h));
    if (!why.empty()) { h->err = fmt("fav_set_ood: %s", why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (fav_status st = refuse_ensemble(h, "fav_set_ood", "an OOD model")) return st;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the new copy first: a failure leaves the handle as it was
    const size_t D = (size_t)m->D, k = (size_t)m->k, R = (size_t)m->R;
    std::vector<float> Pt(D * k), Mt(k * R);
    for (size_t r = 0; r < k; ++r)
        for (size_t j = 0; j < D; ++j) Pt[j * k + r] = m->P[r * D + j];
    for (size_t c = 0; c < R; ++c)
        for (size_t r = 0; r < k; ++r) Mt[r * R + c] = m->M[c * k + r];
    fav_handle::OodDev nw;
    nw.D = m->D; nw.k = m->k; nw.R = m->R; nw.threshold = m->threshold;
    auto upload = [&](void** dst, const void* src, size_t bytes) {
        return hipMalloc(dst, bytes) == hipSuccess && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    const bool ok = upload((void**)&nw.mu, m->mu, D * 4) && upload((void**)&nw.Pt, Pt.data(), D * k * 4) &&
                    upload((void**)&nw.Mt, Mt.data(), k * R * 4) && upload((void**)&nw.cls, m->class_id, R * 4);
    if (!ok) h->err = fmt("fav_set_ood: cannot copy the model to the device: %s", hipGetErrorString(hipGetLastError()));
    return head_commit(h, h->ood, h->ood_on, nw, free_ood, ok);
}

fav_status fav_classify_ood(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                            float* conf, uint8_t* fail, float* score, fav_ood_record* ood, void* stream) {
    return classify_feature_head(h, &fav_handle::ood_on, "fav_classify_ood", "OOD model", "fav_set_ood", images, n, layout, first_index,
                                 labels, conf, fail, score, ood, stream, [&](hipStream_t s) -> const char* {
        const fav_handle::OodDev& o = h->ood;
        launch_ood(h->feat_buf, h->feat_T, h->feat_n, o.D, o.k, o.R, o.mu, o.Pt, o.Mt, o.cls, labels, o.threshold, ood, s);
        return nullptr;
    });
}

// ---- nearest-neighbour OOD scoring (fav_knn.hpp) ----------------------------
namespace {
// What the k-NN head and the patch head need of a workspace before their first launch: the zero bias of bias_floats values, and
// the rows of the bank behind its last whole 64 as a zero-padded tile.  A padded bank (the handle's copy) needs the bias only, once.
fav_status bank_prepare(void* zero_bias, int bias_floats, void* tile, const void* bank, int D, int N, bool padded_bank, hipStream_t s) {
    if (hipMemsetAsync(zero_bias, 0, (size_t)bias_floats * 4, s) != hipSuccess) return FAV_ERR_HIP;
    const int rest = N % 64;
    if (rest == 0 || padded_bank) return FAV_OK;
    const size_t row = (size_t)D * 2;
    if (hipMemsetAsync((char*)tile + rest * row, 0, (size_t)(64 - rest) * row, s) != hipSuccess) return FAV_ERR_HIP;
    if (hipMemcpyAsync(tile, (const char*)bank + (size_t)(N - rest) * row, rest * row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FAV_ERR_HIP;
    return FAV_OK;
}
fav_status knn_prepare(const KnnWs& w, void* ws, const void* bank, int D, int N, bool padded_bank, hipStream_t s) {
    return bank_prepare((char*)ws + w.bias, w.Npad, (char*)ws + w.tile, bank, D, N, padded_bank, s);
}

// The similarity GEMM of the k-NN head and the patch head: q [n][D] bf16 against `cols` rows of a bank (a multiple of 64) as a
// 1x1 convolution over n one-pixel frames, fp32 output into y (row pitch ldy), a zero bias - the production accumulator
const char* sim_gemm(const void* q, int n, int D, const void* rows, const float* zero_bias, float* y, int cols, int ldy, hipStream_t s) {
    fav_conv_desc d;
    memset(&d, 0, sizeof d);
    d.x = q; d.w = rows; d.bias = zero_bias; d.y = y;
    d.n_frames = n; d.H = 1; d.W = 1; d.Cin = D; d.Cout = cols;
    d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0; d.relu = 0; d.out_f32 = 1; d.math_mode = FAV_MATH_BF16;
    d.drop.site = -1;
    return launch_conv(nullptr, d, cols, ldy, false, Group{}, s);
}

// The head on a prepared workspace: the query kernel, the GEMM (one launch; two when an unpadded bank ends in a part tile),
// the select.  The arguments have been checked (knn_dims_error, the pointers).  Returns the conv launcher's refusal, if any.
const char* launch_knn(const void* feat, int S, int n, int D, const void* bank, int N, int k, const int32_t* cls, float threshold,
                       const KnnWs& w, void* ws, bool padded_bank, fav_knn_record* rec, hipStream_t s) {
    KnnQueryParams qp;
    qp.feat = (const uint16_t*)feat; qp.q = (uint16_t*)((char*)ws + w.q); qp.flags = (int32_t*)((char*)ws + w.flags);
    qp.S = S; qp.n = n; qp.D = D; qp.inv_S = (float)(1.0 / S);
    hipLaunchKernelGGL(knn_query_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, s, qp);
    float* const sim = (float*)((char*)ws + w.sim);
    auto gemm = [&](const void* rows, int col0, int cols) {
        return sim_gemm(qp.q, n, D, rows, (const float*)((char*)ws + w.bias) + col0, sim + col0, cols, w.Npad, s);
    };
    const int whole = padded_bank ? w.Npad : (N & ~63);
    if (whole > 0)
        if (const char* e = gemm(bank, 0, whole)) return e;
    if (whole < w.Npad)
        if (const char* e = gemm((const char*)ws + w.tile, whole, 64)) return e;
    KnnSelectParams sp;
    sp.sim = sim; sp.flags = qp.flags; sp.cls = cls; sp.rec = (int32_t*)rec;
    sp.N = N; sp.ld = w.Npad; sp.k = k; sp.threshold = threshold;
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)n), dim3(KNN_SEL_THREADS), 0, s, sp);
    return nullptr;
}

void free_knn(fav_handle::KnnDev* o) {
    for (void* q : {o->bank, o->ws, (void*)o->cls}) if (q) (void)hipFree(q);
    *o = fav_handle::KnnDev{};
}
}  // namespace

fav_status fav_check_knn_bank(const fav_knn_bank* b, int32_t D_expected, char* err, size_t err_cap) {
    static_assert(sizeof(fav_knn_record) == 24, "fav_knn_record is 6 dwords");
    return check_reply(knn_bank_error(b, D_expected), err, err_cap);
}

size_t fav_knn_workspace_bytes(int32_t n, int32_t D, int32_t N) {
    if (n < 1 || !knn_dims_error(D, N, 1).empty()) return 0;
    return knn_workspace(n, D, N, false).bytes;
}

fav_status fav_set_knn(fav_handle* h, const fav_knn_bank* b) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!b) return head_clear(h, h->knn, h->knn_on, free_knn);
    const std::string why = knn_bank_error(b, feature_width(h));
    if (!why.empty()) { h->err = fmt("fav_set_knn: %s", why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (fav_status st = refuse_ensemble(h, "fav_set_knn", "a k-NN bank")) return st;
    const KnnWs w = knn_workspace(h->cfg.max_batch, b->D, b->N, true);
    if (w.bytes > KNN_MAX_WS_BYTES) {
        h->err = fmt("fav_set_knn: the workspace of max_batch=%d frames against N=%d rows (%d padded) is %zu bytes, above the limit of %zu",
                     (int)h->cfg.max_batch, b->N, w.Npad, w.bytes, KNN_MAX_WS_BYTES);
        return FAV_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the new copy first: a failure leaves the handle as it was
    fav_handle::KnnDev nw;
    nw.D = b->D; nw.N = b->N; nw.k = b->k; nw.threshold = b->threshold;
    const size_t row = (size_t)b->D * 2, bank_bytes = (size_t)b->N * row, pad_bytes = (size_t)(w.Npad - b->N) * row;
    bool ok = hipMalloc(&nw.bank, (size_t)w.Npad * row) == hipSuccess && hipMalloc(&nw.ws, w.bytes) == hipSuccess &&
              hipMemcpy(nw.bank, b->rows, bank_bytes, hipMemcpyHostToDevice) == hipSuccess &&
              (pad_bytes == 0 || hipMemset((char*)nw.bank + bank_bytes, 0, pad_bytes) == hipSuccess);
    if (ok && b->class_id)
        ok = hipMalloc((void**)&nw.cls, (size_t)b->N * 4) == hipSuccess && hipMemcpy(nw.cls, b->class_id, (size_t)b->N * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && knn_prepare(w, nw.ws, nw.bank, b->D, b->N, true, nullptr) == FAV_OK && hipStreamSynchronize(nullptr) == hipSuccess;
    if (!ok) h->err = fmt("fav_set_knn: cannot copy the bank to the device: %s", hipGetErrorString(hipGetLastError()));
    return head_commit(h, h->knn, h->knn_on, nw, free_knn, ok);
}

fav_status fav_classify_knn(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                            float* conf, uint8_t* fail, float* score, fav_knn_record* knn, void* stream) {
    return classify_feature_head(h, &fav_handle::knn_on, "fav_classify_knn", "k-NN bank", "fav_set_knn", images, n, layout, first_index,
                                 labels, conf, fail, score, knn, stream, [&](hipStream_t s) {
        const fav_handle::KnnDev& o = h->knn;
        const KnnWs w = knn_workspace(h->cfg.max_batch, o.D, o.N, true);
        return launch_knn(h->feat_buf, h->feat_T, h->feat_n, o.D, o.bank, o.N, o.k, o.cls, o.threshold, w, o.ws, true, knn, s);
    });
}

// ---- window-level drift detection (fav_drift.hpp) ---------------------------
namespace {
// The test on a prepared workspace (the pool's reference rows, its zero rows and the zero bias are there; with cached_ref
// also the reference's block of U and its diagonal): the query kernel, one GEMM, the quantise, row-sum, permutation and final
// kernels.  The arguments have been checked (drift_dims_error, the pointers).  Returns the conv launcher's refusal, if any.
const char* drift_gemm(const DriftWs& w, void* ws, int D, int row0, int rows, int cols, int ldg, float* G, hipStream_t s) {
    fav_conv_desc d;
    memset(&d, 0, sizeof d);
    d.x = (const char*)ws + w.pool + (size_t)row0 * D * 2; d.w = (const char*)ws + w.pool;
    d.bias = (const float*)((char*)ws + w.bias); d.y = G;
    d.n_frames = rows; d.H = 1; d.W = 1; d.Cin = D; d.Cout = cols;
    d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0; d.relu = 0; d.out_f32 = 1; d.math_mode = FAV_MATH_BF16;
    d.drop.site = -1;
    return launch_conv(nullptr, d, cols, ldg, false, Group{}, s);
}
void drift_quant(const DriftWs& w, void* ws, int row0, int rows, const float* G, int ldg, hipStream_t s) {
    DriftQuantParams qp;
    qp.G = G; qp.diag = (float*)((char*)ws + w.diag); qp.U = (uint32_t*)((char*)ws + w.U);
    qp.row0 = row0; qp.rows = rows; qp.ldg = ldg; qp.ldu = w.ld;
    hipLaunchKernelGGL(drift_quant_kernel, dim3((unsigned)rows), dim3(256), 0, s, qp);
}
const char* launch_drift(const void* feat, int S, int n, int D, int R, int n_perm, uint64_t seed, float alpha, const DriftWs& w,
                         void* ws, bool cached_ref, fav_drift_record* rec, int64_t* perm_sums, hipStream_t s) {
    const int Np = R + n;
    KnnQueryParams qp;
    qp.feat = (const uint16_t*)feat; qp.q = (uint16_t*)((char*)ws + w.pool) + (size_t)R * D; qp.flags = (int32_t*)((char*)ws + w.flags);
    qp.S = S; qp.n = n; qp.D = D; qp.inv_S = (float)(1.0 / S);
    hipLaunchKernelGGL(knn_query_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, s, qp);
    float* const G = (float*)((char*)ws + w.G);
    const int row0 = cached_ref ? R : 0, rows = Np - row0;
    if (const char* e = drift_gemm(w, ws, D, row0, rows, (Np + 63) & ~63, w.ld, G, s)) return e;
    drift_quant(w, ws, row0, rows, G, w.ld, s);
    long long* const r = (long long*)((char*)ws + w.r);
    hipLaunchKernelGGL(drift_rowsum_kernel, dim3((unsigned)((Np + 3) / 4)), dim3(256), 0, s, (const uint32_t*)((char*)ws + w.U), r, Np, w.ld);
    DriftPermParams pp;
    pp.U = (const uint32_t*)((char*)ws + w.U); pp.r = r; pp.flags = qp.flags;
    pp.sums = (long long*)((char*)ws + w.sums); pp.user_sums = (long long*)perm_sums;
    pp.R = R; pp.n = n; pp.Np = Np; pp.ld = w.ld; pp.P = n_perm;
    pp.sort_n = 4;
    while (pp.sort_n < Np) pp.sort_n <<= 1;
    pp.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull); pp.seed_hi = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(drift_perm_kernel, dim3((unsigned)(n_perm + 1)), dim3(DRIFT_PERM_THREADS), 0, s, pp);
    DriftFinalParams fp;
    fp.r = r; fp.sums = pp.sums; fp.flags = qp.flags; fp.rec = (unsigned long long*)rec;
    fp.R = R; fp.n = n; fp.Np = Np; fp.P = n_perm; fp.alpha = alpha;
    hipLaunchKernelGGL(drift_final_kernel, dim3(1), dim3(DRIFT_FINAL_THREADS), 0, s, fp);
    return nullptr;
}

void free_drift(fav_handle::DriftDev* o) {
    if (o->ws) (void)hipFree(o->ws);
    *o = fav_handle::DriftDev{};
}
}  // namespace

fav_status fav_check_drift_ref(const fav_drift_ref* b, int32_t D_expected, char* err, size_t err_cap) {
    static_assert(sizeof(fav_drift_record) == 48 && alignof(fav_drift_record) == 8, "fav_drift_record is six 8-byte words");
    return check_reply(drift_ref_error(b, D_expected), err, err_cap);
}

size_t fav_drift_workspace_bytes(int32_t n, int32_t D, int32_t R, int32_t n_perm) {
    if (!drift_dims_error(D, R, n_perm, 0.f, &n).empty()) return 0;
    return drift_workspace(n, D, R, n_perm, false).bytes;
}

fav_status fav_set_drift(fav_handle* h, const fav_drift_ref* b) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!b) return head_clear(h, h->drift, h->drift_on, free_drift);
    const std::string why = drift_ref_error(b, feature_width(h));
    if (!why.empty()) { h->err = fmt("fav_set_drift: %s", why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (fav_status st = refuse_ensemble(h, "fav_set_drift", "a drift reference")) return st;
    if (h->cfg.max_batch < 2 || h->cfg.max_batch > DRIFT_MAX_N) {
        h->err = fmt("fav_set_drift: max_batch=%d outside [2, %d]: a window is 2 to %d frames", (int)h->cfg.max_batch, DRIFT_MAX_N, DRIFT_MAX_N);
        return FAV_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the new copy first: a failure leaves the handle as it was
    const DriftWs w = drift_workspace(h->cfg.max_batch, b->D, b->R, b->n_perm, true);
    fav_handle::DriftDev nw;
    nw.D = b->D; nw.R = b->R; nw.n_perm = b->n_perm; nw.seed = b->seed; nw.alpha = b->alpha;
    const int Rpad = (b->R + 63) & ~63;
    float* G = nullptr;
    bool ok = hipMalloc(&nw.ws, w.bytes) == hipSuccess && hipMalloc((void**)&G, (size_t)b->R * Rpad * 4) == hipSuccess &&
              hipMemset((char*)nw.ws + w.pool, 0, (size_t)w.ld * b->D * 2) == hipSuccess &&
              hipMemset((char*)nw.ws + w.bias, 0, (size_t)w.ld * 4) == hipSuccess &&
              hipMemcpy((char*)nw.ws + w.pool, b->rows, (size_t)b->R * b->D * 2, hipMemcpyHostToDevice) == hipSuccess;
    const char* e = nullptr;
    if (ok) {
        // the reference's own block of distances, once: R rows against pad64(R) rows of the pool
        e = drift_gemm(w, nw.ws, b->D, 0, b->R, Rpad, Rpad, G, nullptr);
        route_clear();
        if (!e) drift_quant(w, nw.ws, 0, b->R, G, Rpad, nullptr);
        ok = !e && hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    }
    if (G) (void)hipFree(G);
    if (!ok) h->err = e ? fmt("fav_set_drift: %s", e) : fmt("fav_set_drift: cannot copy the reference to the device: %s", hipGetErrorString(hipGetLastError()));
    return head_commit(h, h->drift, h->drift_on, nw, free_drift, ok);
}

fav_status fav_classify_drift(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                              float* conf, uint8_t* fail, float* score, fav_drift_record* drift, void* stream) {
    if (h && h->drift_on && n < 2) {
        route_clear();
        h->err = fmt("fav_classify_drift: n=%d is below 2: a window needs two frames", (int)n);
        return FAV_ERR_INVALID_ARG;
    }
    return classify_feature_head(h, &fav_handle::drift_on, "fav_classify_drift", "drift reference", "fav_set_drift", images, n, layout,
                                 first_index, labels, conf, fail, score, drift, stream, [&](hipStream_t s) {
        const fav_handle::DriftDev& o = h->drift;
        const DriftWs w = drift_workspace(h->cfg.max_batch, o.D, o.R, o.n_perm, true);
        return launch_drift(h->feat_buf, h->feat_T, h->feat_n, o.D, o.R, o.n_perm, o.seed, o.alpha, w, o.ws, true, drift, nullptr, s);
    });
}

// ---- class activation maps (fav_cam.hpp) -------------------------------------
namespace {
// The head: one launch, a block a frame, the weight rows and the maps in LDS.  The arguments have been checked
// (cam_dims_error, the pointers).  Returns a refusal of the runtime's, if it has one.
const char* launch_cam(const void* maps, int S, int n, int Hf, int Wf, int C, const void* w, long long ldw, const float* bias,
                       int n_classes, const int32_t* classes, int K, float* cam, fav_cam_record* rec, hipStream_t s) {
    CamParams p;
    p.maps = (const uint16_t*)maps; p.w = (const uint16_t*)w; p.bias = bias; p.classes = classes; p.cam = cam; p.rec = (int32_t*)rec;
    p.S = S; p.n = n; p.HW = Hf * Wf; p.Wf = Wf; p.C = C; p.K = K; p.n_classes = n_classes; p.ldw = ldw;
    p.inv_S = (float)(1.0 / S); p.inv_HW = (float)(1.0 / (Hf * Wf));
    const size_t lds = (size_t)K * C * 2 + (size_t)K * p.HW * 4;     // at most 96 KB
    void (*const fn)(const CamParams) = K == 1 ? cam_kernel<1> : cam_kernel<CAM_MAX_K>;
    if (lds + CAM_STATIC_LDS > 64 * 1024) {      // the kernel's static LDS counts towards the default limit too
        static DeviceFlags attr_set[2];   // hipFuncSetAttribute applies to the CURRENT device only
        DeviceFlags& done = attr_set[K == 1 ? 0 : 1];
        if (!done.test_current()) {
            if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
                return "cannot reserve LDS for the weight rows and the maps";
            done.set_current();
        }
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)n), dim3(CAM_THREADS), lds, s, p);
    return nullptr;
}

void launch_cam_heatmap(const float* cam, const fav_cam_record* rec, int m, int Hf, int Wf, int H, int W, uint8_t* out, hipStream_t s) {
    CamHeatParams p;
    p.cam = cam; p.rec = (const int32_t*)rec; p.out = out; p.m = m; p.Hf = Hf; p.Wf = Wf; p.H = H; p.W = W;
    p.scale_y = (float)Hf / (float)H; p.scale_x = (float)Wf / (float)W;
    hipLaunchKernelGGL(cam_heatmap_kernel, dim3(grid_for((long long)m * H * W)), dim3(256), 0, s, p);
}

// the row pitch of the fc's weights: the last layer of the plan, whose rows the head reads
int fc_pitch(const fav_handle* h) { return h->plan.layers.back().k; }

// the head's own ranges on a handle whose map tap is on, and its launch on the maps the tap holds
extern "C++" std::string cam_handle_dims_error(const fav_handle* h, int K) {
    return cam_dims_error(h->map.S, 1, h->map.Hf, h->map.Wf, h->map.C, fc_pitch(h), h->cfg.num_classes, K);
}
const char* cam_on_tap(const fav_handle* h, const int32_t* classes, int K, float* cam, fav_cam_record* rec, hipStream_t s) {
    const size_t fc = h->plan.layers.size() - 1;
    return launch_cam(h->map_tap.buf, h->map_tap.S, h->map_tap.n, h->map.Hf, h->map.Wf, h->map.C, h->weights[fc].w_m[0], fc_pitch(h),
                      h->weights[fc].b_m[0], h->cfg.num_classes, classes, K, cam, rec, s);
}
bool bad_cam_buffers(const void* classes, const void* cam, const void* rec) {
    return !classes || !cam || !rec || ((uintptr_t)classes & 3) || ((uintptr_t)cam & 3) || ((uintptr_t)rec & 7);
}
}  // namespace

fav_status fav_map_tap_info(const fav_config* cfg, size_t* bytes, int32_t* s_map, int32_t* hf, int32_t* wf, int32_t* c, char* err,
                            size_t err_cap) {
    return tap_info("fav_map_tap_info", cfg, map_tap_unsupported, true, err, err_cap, [&](std::string* why) -> fav_status {
        Plan P;
        if (fav_status st = plan_resnet(*cfg, 1, false, &P, why)) return st;
        const MapTapDims d = map_tap_dims(P, cfg->max_batch);
        if (bytes) *bytes = d.bytes;
        put_sizes({{s_map, d.S}, {hf, d.Hf}, {wf, d.Wf}, {c, d.C}});
        return FAV_OK;
    });
}

fav_status fav_set_map_tap(fav_handle* h, int32_t enable, size_t max_bytes) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!enable) return tap_off(h, h->map_tap);
    return tap_on(h, "fav_set_map_tap", h->map_tap, h->map, map_tap_unsupported(h->cfg.arch, h->n_members, h->cfg.math_mode),
                  "maps of max_batch frames take", max_bytes, CAM_DEFAULT_BUDGET, [&] { return map_tap_dims(h->plan, h->cfg.max_batch); });
}

fav_status fav_get_maps(fav_handle* h, void* out, int32_t* s_out, int32_t* n_out, int32_t* hf_out, int32_t* wf_out, int32_t* c_out,
                        void* stream) {
    if (!h) return FAV_ERR_INVALID_ARG;
    const fav_handle::LocTap& t = h->map_tap;
    const MapTapDims& d = h->map;
    return tap_get(h, "fav_get_maps", kMapWords, t, {{s_out, t.S}, {n_out, t.n}, {hf_out, d.Hf}, {wf_out, d.Wf}, {c_out, d.C}}, out,
                   (size_t)t.S * t.n * d.Hf * d.Wf * d.C * 2, stream);
}

// ---- the stage tap (fav_cam.hpp stage_tap_dims): the map tap's steps on the output of a residual stage's last block
fav_status fav_stage_tap_info(const fav_config* cfg, int32_t stage, size_t* bytes, int32_t* s_map, int32_t* hf, int32_t* wf, int32_t* c,
                              char* err, size_t err_cap) {
    return tap_info("fav_stage_tap_info", cfg, map_tap_unsupported, true, err, err_cap, [&](std::string* why) -> fav_status {
        if (stage < 1 || stage > 4) { *why = fmt("stage=%d outside [1, 4]", stage); return FAV_ERR_INVALID_ARG; }
        Plan P;
        if (fav_status st = plan_resnet(*cfg, 1, false, &P, why)) return st;
        const MapTapDims d = stage_tap_dims(P, cfg->max_batch, stage);
        if (bytes) *bytes = d.bytes;
        put_sizes({{s_map, d.S}, {hf, d.Hf}, {wf, d.Wf}, {c, d.C}});
        return FAV_OK;
    });
}

fav_status fav_set_stage_tap(fav_handle* h, int32_t stage, size_t max_bytes) {
    if (!h) return FAV_ERR_INVALID_ARG;
    const char* fn = "fav_set_stage_tap";
    if (stage == 0) {
        h->stage_no = 0;
        return tap_off(h, h->stage_tap);
    }
    if (stage < 0 || stage > 4) { h->err = fmt("%s: stage=%d outside [0, 4]", fn, stage); return FAV_ERR_INVALID_ARG; }
    if (const char* why = map_tap_unsupported(h->cfg.arch, h->n_members, h->cfg.math_mode)) { h->err = fmt("%s: %s", fn, why); return FAV_ERR_UNSUPPORTED; }
    const MapTapDims d = stage_tap_dims(h->plan, h->cfg.max_batch, stage);
    const char* what = "stage maps of max_batch frames take";
    std::string why = d.op < 0 ? fmt("the plan has no stage %d", stage) : patch_map_error(h->cfg.max_batch, d.Hf, d.Wf);
    if (!why.empty()) why = fmt("stage %d: %s", stage, why.c_str());
    if (why.empty()) why = tap_budget_error(what, d.bytes, max_bytes, CAM_DEFAULT_BUDGET);
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    if (h->stage_tap.on && h->stage_no != stage) {              // another stage: the buffer goes once what is enqueued has run
        h->stage_no = 0;
        if (fav_status st = tap_off(h, h->stage_tap)) return st;
    }
    if (fav_status st = tap_on(h, fn, h->stage_tap, h->stage, nullptr, what, max_bytes, CAM_DEFAULT_BUDGET, [&] { return d; })) return st;
    h->stage_no = stage;
    return FAV_OK;
}

fav_status fav_get_stage_maps(fav_handle* h, void* out, int32_t* stage_out, int32_t* s_out, int32_t* n_out, int32_t* hf_out,
                              int32_t* wf_out, int32_t* c_out, void* stream) {
    if (!h) return FAV_ERR_INVALID_ARG;
    const fav_handle::LocTap& t = h->stage_tap;
    const MapTapDims& d = h->stage;
    return tap_get(h, "fav_get_stage_maps", kStageWords, t,
                   {{stage_out, h->stage_no}, {s_out, t.S}, {n_out, t.n}, {hf_out, d.Hf}, {wf_out, d.Wf}, {c_out, d.C}}, out,
                   (size_t)t.S * t.n * d.Hf * d.Wf * d.C * 2, stream);
}

fav_status fav_cam(fav_handle* h, const int32_t* classes, int32_t K, float* cam, fav_cam_record* rec, void* stream) {
    static_assert(sizeof(fav_cam_record) == 32, "fav_cam_record is 8 dwords");
    return map_head_on_last_call(h, "fav_cam", kMapWords, &fav_handle::map_tap, bad_cam_buffers(classes, cam, rec),
                                 [&] { return cam_handle_dims_error(h, K); }, stream,
                                 [&](hipStream_t s) { return cam_on_tap(h, classes, K, cam, rec, s); });
}

fav_status fav_classify_cam(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                            float* conf, uint8_t* fail, float* score, float* cam, fav_cam_record* rec, void* stream) {
    return classify_map_head(h, "fav_classify_cam", kMapWords, &fav_handle::map_tap, bad_cam_buffers(labels, cam, rec),
                             [&] { return cam_handle_dims_error(h, 1); }, images, n, layout, first_index, labels, conf, fail, score, stream,
                             [&](hipStream_t s) { return cam_on_tap(h, labels, 1, cam, rec, s); });
}

// ---- attention rollout (fav_rollout.hpp) ---------------------------------------
namespace {
// The head: one launch, a block a frame.  The arguments have been checked (rollout_dims_error, the pointers).
void launch_rollout(const float* a, long long layer_stride, int L, int n, int gh, int gw, int ld, int first_layer, float* map,
                    fav_rollout_record* rec, hipStream_t s) {
    RolloutParams p;
    p.a = a; p.map = map; p.rec = (int32_t*)rec; p.layer_stride = layer_stride;
    p.L = L; p.T = gh * gw + 1; p.gw = gw; p.ld = ld; p.first_layer = first_layer;
    hipLaunchKernelGGL(attn_rollout_kernel, dim3((unsigned)n), dim3(ROLL_THREADS), 0, s, p);
}
// the patch grid of a ViT handle
void vit_grid(const fav_handle* h, int* gh, int* gw) {
    const VitDef& V = kVit[h->cfg.arch - 2];
    *gh = h->cfg.in_h / V.patch; *gw = h->cfg.in_w / V.patch;
}
// the head's own ranges on a handle whose attention tap is on, and its launch on the attention the tap holds
extern "C++" std::string rollout_handle_dims_error(const fav_handle* h, int first_layer) {
    int gh, gw;
    vit_grid(h, &gh, &gw);
    return rollout_dims_error(h->attn.L, 1, gh, gw, h->attn.ld, first_layer);
}
const char* rollout_on_tap(const fav_handle* h, int first_layer, float* map, fav_rollout_record* rec, hipStream_t s) {
    int gh, gw;
    vit_grid(h, &gh, &gw);
    const int n = h->attn_tap.n;
    launch_rollout((const float*)h->attn_tap.buf, (long long)n * h->attn.T * h->attn.ld, h->attn.L, n, gh, gw, h->attn.ld, first_layer, map, rec, s);
    return nullptr;
}
bool bad_rollout_buffers(const void* map, const void* rec) { return !map || !rec || ((uintptr_t)map & 3) || ((uintptr_t)rec & 7); }
}  // namespace

fav_status fav_attn_tap_info(const fav_config* cfg, size_t* bytes, int32_t* layers, int32_t* tokens, int32_t* ld, char* err, size_t err_cap) {
    return tap_info("fav_attn_tap_info", cfg, attn_tap_unsupported, false, err, err_cap, [&](std::string* why) -> fav_status {
        Plan P;
        if (fav_status st = plan_vit(*cfg, &P, why)) return st;
        const AttnTapDims d = attn_tap_dims(kVit[cfg->arch - 2].depth, P.ntok, cfg->max_batch);
        if (bytes) *bytes = d.bytes;
        put_sizes({{layers, d.L}, {tokens, d.T}, {ld, d.ld}});
        return FAV_OK;
    });
}

fav_status fav_set_attn_tap(fav_handle* h, int32_t enable, size_t max_bytes) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!enable) return tap_off(h, h->attn_tap);
    return tap_on(h, "fav_set_attn_tap", h->attn_tap, h->attn, attn_tap_unsupported(h->cfg.arch, h->n_members, h->cfg.math_mode),
                  "attention of max_batch frames takes", max_bytes, ATTN_TAP_DEFAULT_BUDGET,
                  [&] { return attn_tap_dims(kVit[h->cfg.arch - 2].depth, h->plan.ntok, h->cfg.max_batch); });
}

fav_status fav_get_attention(fav_handle* h, float* out, int32_t* l_out, int32_t* n_out, int32_t* t_out, int32_t* ld_out, void* stream) {
    if (!h) return FAV_ERR_INVALID_ARG;
    const fav_handle::LocTap& t = h->attn_tap;
    const AttnTapDims& d = h->attn;
    return tap_get(h, "fav_get_attention", kAttnWords, t, {{l_out, d.L}, {n_out, t.n}, {t_out, d.T}, {ld_out, d.ld}}, out,
                   (size_t)d.L * t.n * d.T * d.ld * 4, stream);
}

fav_status fav_rollout(fav_handle* h, int32_t first_layer, float* map, fav_rollout_record* rec, void* stream) {
    static_assert(sizeof(fav_rollout_record) == 32, "fav_rollout_record is 8 dwords");
    static_assert(offsetof(fav_rollout_record, peak) == offsetof(fav_cam_record, peak) && offsetof(fav_rollout_record, floor) == offsetof(fav_cam_record, floor),
                  "fav_op_cam_heatmap reads peak and floor of either record");
    return map_head_on_last_call(h, "fav_rollout", kAttnWords, &fav_handle::attn_tap, bad_rollout_buffers(map, rec),
                                 [&] { return rollout_handle_dims_error(h, first_layer); }, stream,
                                 [&](hipStream_t s) { return rollout_on_tap(h, first_layer, map, rec, s); });
}

fav_status fav_classify_rollout(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                                float* conf, uint8_t* fail, float* score, int32_t first_layer, float* map, fav_rollout_record* rec,
                                void* stream) {
    return classify_map_head(h, "fav_classify_rollout", kAttnWords, &fav_handle::attn_tap, bad_rollout_buffers(map, rec),
                             [&] { return rollout_handle_dims_error(h, first_layer); }, images, n, layout, first_index, labels, conf, fail,
                             score, stream, [&](hipStream_t s) { return rollout_on_tap(h, first_layer, map, rec, s); });
}

// ---- patch-level anomaly maps (fav_patch.hpp) -----------------------------------
namespace {
// bank_prepare on the head's workspace: the zero bias serves every chunk
fav_status patch_prepare(const PatchWs& w, void* ws, const void* bank, int D, int N, bool padded_bank, hipStream_t s) {
    return bank_prepare((char*)ws + w.bias, w.chunk, (char*)ws + w.tile, bank, D, N, padded_bank, s);
}

// The head on a prepared workspace: the query kernel, a cell a block; per column chunk of the bank the GEMM into the slab (two
// launches where an unpadded bank's part tile falls into the chunk) and the fold of the slab; the score kernel, a frame a
// block.  Stream order makes reusing the slab safe.  The arguments have been checked (patch_map_error, knn_dims_error, the
// pointers).  radius < 0: the k-NN head's query kernel, as it stands; 0 .. 2: the caller asked for a site, the locally aware
// query (patch_query_error has passed, maps is 16-byte aligned).  Returns the conv launcher's refusal, if any.
void launch_patch_query(const void* maps, int S, int n, int Hf, int Wf, int C, int radius, void* q, int32_t* flags, hipStream_t s) {
    PatchQueryParams p;
    p.maps = (const uint16_t*)maps; p.q = (uint16_t*)q; p.flags = flags;
    p.S = S; p.n = n; p.Hf = Hf; p.Wf = Wf; p.C = C; p.CS = patch_query_slice(Wf, C); p.inv_S = (float)(1.0 / S);
    void (*const fn)(const PatchQueryParams) = radius == 0 ? patch_local_query_kernel<0, 4> : radius == 1 ? patch_local_query_kernel<1, 2>
                                                                                                       : patch_local_query_kernel<2, 1>;
    const size_t lds = (size_t)Wf * (p.CS + PQ_PAD) * 4;      // at most PQ_LDS_BYTES
    hipLaunchKernelGGL(fn, dim3((unsigned)(n * Hf)), dim3(PQ_THREADS), lds, s, p);
}
const char* launch_patch(const void* maps, int S, int n, int Hf, int Wf, int C, int radius, const void* bank, int N, float threshold,
                         const PatchWs& w, void* ws, bool padded_bank, float* dist, int32_t* row, fav_patch_record* rec, hipStream_t s) {
    const int HW = Hf * Wf, M = n * HW;
    KnnQueryParams qp;
    qp.feat = (const uint16_t*)maps; qp.q = (uint16_t*)((char*)ws + w.q); qp.flags = (int32_t*)((char*)ws + w.flags);
    qp.S = S; qp.n = M; qp.D = C; qp.inv_S = (float)(1.0 / S);
    if (radius < 0) hipLaunchKernelGGL(knn_query_kernel, dim3((unsigned)M), dim3(KNN_THREADS), 0, s, qp);
    else launch_patch_query(maps, S, n, Hf, Wf, C, radius, qp.q, qp.flags, s);
    float* const slab = (float*)((char*)ws + w.slab);
    const float* const zero_bias = (const float*)((char*)ws + w.bias);
    const int whole = padded_bank ? w.Npad : (N & ~63);        // the rows the GEMM reads in place
    PatchFoldParams fp;
    fp.sim = slab; fp.flags = qp.flags; fp.best = (uint2*)((char*)ws + w.best); fp.M = M; fp.ld = w.chunk;
    for (int c0 = 0; c0 < w.Npad; c0 += w.chunk) {
        const int cols = std::min(w.chunk, w.Npad - c0), in_place = std::max(0, std::min(cols, whole - c0));
        if (in_place > 0)
            if (const char* e = sim_gemm(qp.q, M, C, (const char*)bank + (size_t)c0 * C * 2, zero_bias, slab, in_place, w.chunk, s)) return e;
        if (in_place < cols)
            if (const char* e = sim_gemm(qp.q, M, C, (const char*)ws + w.tile, zero_bias, slab + in_place, 64, w.chunk, s)) return e;
        fp.cols = std::min(cols, N - c0); fp.row0 = c0; fp.first = c0 == 0 ? 1 : 0;
        hipLaunchKernelGGL(patch_fold_kernel, dim3((unsigned)((M + PATCH_FOLD_ROWS - 1) / PATCH_FOLD_ROWS)), dim3(PATCH_FOLD_THREADS), 0, s, fp);
    }
    PatchScoreParams sp;
    sp.best = fp.best; sp.flags = qp.flags; sp.dist = dist; sp.row = row; sp.rec = (int32_t*)rec;
    sp.HW = HW; sp.Wf = Wf; sp.threshold = threshold; sp.inv_HW = (float)(1.0 / HW);
    hipLaunchKernelGGL(patch_score_kernel, dim3((unsigned)n), dim3(PATCH_SCORE_THREADS), 0, s, sp);
    return nullptr;
}

void free_patch(fav_handle::PatchDev* o) {
    for (void* q : {o->bank, o->ws}) if (q) (void)hipFree(q);
    *o = fav_handle::PatchDev{};
}
bool bad_patch_buffers(const void* dist, const void* row, const void* rec) {
    return !dist || !rec || ((uintptr_t)dist & 3) || ((uintptr_t)row & 3) || ((uintptr_t)rec & 7);
}
// what the head's two entry points refuse once the tap is known to be on, and its launch on the maps the tap holds
extern "C++" std::string patch_handle_error(const fav_handle* h) {
    return h->patch_on ? std::string() : std::string("no patch bank set (fav_set_patch_bank)");
}
const char* patch_on_tap(const fav_handle* h, float* dist, int32_t* row, fav_patch_record* rec, hipStream_t s) {
    const fav_handle::PatchDev& o = h->patch;
    const PatchWs w = patch_workspace((long long)h->cfg.max_batch * o.Hf * o.Wf, o.D, o.N, o.chunk_rows, true);
    const fav_handle::LocTap& t = o.stage > 0 ? h->stage_tap : h->map_tap;
    return launch_patch(t.buf, t.S, t.n, o.Hf, o.Wf, o.D, o.radius, o.bank, o.N, o.threshold, w, o.ws, true, dist, row, rec, s);
}
// a bank at a site reads the stage tap, which must be at the bank's stage (empty: nothing to say - a plain bank, or no bank)
extern "C++" std::string patch_stage_error(const fav_handle* h) {
    const int tap = h->stage_tap.on ? h->stage_no : 0;
    if (!h->patch_on || h->patch.stage == 0 || tap == h->patch.stage) return std::string();
    return fmt("the bank is at stage %d, the stage tap at stage %d (0: off; fav_set_stage_tap)", h->patch.stage, tap);
}
}  // namespace

fav_status fav_check_patch_bank(const fav_patch_bank* b, int32_t D_expected, char* err, size_t err_cap) {
    static_assert(sizeof(fav_patch_record) == 32, "fav_patch_record is 8 dwords");
    static_assert(offsetof(fav_patch_record, peak) == offsetof(fav_cam_record, peak) && offsetof(fav_patch_record, floor) == offsetof(fav_cam_record, floor),
                  "fav_op_cam_heatmap reads peak and floor of either record");
    return check_reply(patch_bank_error(b, D_expected), err, err_cap);
}

size_t fav_patch_workspace_bytes(int32_t cells_total, int32_t D, int32_t N, int32_t chunk_rows) {
    if (cells_total < 1 || !knn_dims_error(D, N, 1).empty() || !patch_chunk_error(chunk_rows).empty()) return 0;
    return patch_workspace(cells_total, D, N, chunk_rows, false).bytes;
}

int32_t fav_patch_chunk_rows(int32_t cells_total, int32_t N, int32_t chunk_rows) {
    if (cells_total < 1 || N < 1 || N > KNN_MAX_N || !patch_chunk_error(chunk_rows).empty()) return 0;
    return patch_chunk(cells_total, N, chunk_rows);
}

namespace {
// fav_set_patch_bank (site NULL) and fav_set_patch_bank_at: `fn` is the name the messages carry
fav_status set_patch_bank(fav_handle* h, const fav_patch_bank* b, const fav_patch_site* site, const char* fn) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!b) {
        if (!h->patch_on) return FAV_OK;
        if (fav_status st = wait_enqueued(h)) return st;
        free_patch(&h->patch);
        h->patch_on = false;
        return FAV_OK;
    }
    if (const char* why = map_tap_unsupported(h->cfg.arch, h->n_members, h->cfg.math_mode)) {
        h->err = fmt("%s: %s", fn, why);
        return FAV_ERR_UNSUPPORTED;
    }
    std::string why = site ? patch_site_error(site) : std::string();
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    const MapTapDims d = site ? stage_tap_dims(h->plan, h->cfg.max_batch, site->stage) : map_tap_dims(h->plan, h->cfg.max_batch);
    why = patch_bank_error(b, d.C);
    if (why.empty()) why = patch_map_error(h->cfg.max_batch, d.Hf, d.Wf);
    if (!why.empty()) { h->err = fmt("%s: %s", fn, why.c_str()); return FAV_ERR_INVALID_ARG; }
    const long long cells = (long long)h->cfg.max_batch * d.Hf * d.Wf;
    const PatchWs w = patch_workspace(cells, b->D, b->N, b->chunk_rows, true);
    if (w.bytes > PATCH_MAX_WS_BYTES) {
        h->err = fmt("%s: the workspace of max_batch=%d frames of %d x %d cells against N=%d rows in chunks of %d is %zu bytes, "
                     "above the limit of %zu", fn, (int)h->cfg.max_batch, d.Hf, d.Wf, b->N, w.chunk, w.bytes, PATCH_MAX_WS_BYTES);
        return FAV_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the new copy first: a failure leaves the handle as it was
    fav_handle::PatchDev nw;
    nw.D = b->D; nw.N = b->N; nw.chunk_rows = b->chunk_rows; nw.Hf = d.Hf; nw.Wf = d.Wf; nw.threshold = b->threshold;
    if (site) { nw.stage = site->stage; nw.radius = site->radius; }
    const size_t row = (size_t)b->D * 2, bank_bytes = (size_t)b->N * row, pad_bytes = (size_t)(w.Npad - b->N) * row;
    bool ok = hipMalloc(&nw.bank, (size_t)w.Npad * row) == hipSuccess && hipMalloc(&nw.ws, w.bytes) == hipSuccess &&
              hipMemcpy(nw.bank, b->rows, bank_bytes, hipMemcpyHostToDevice) == hipSuccess &&
              (pad_bytes == 0 || hipMemset((char*)nw.bank + bank_bytes, 0, pad_bytes) == hipSuccess);
    ok = ok && patch_prepare(w, nw.ws, nw.bank, b->D, b->N, true, nullptr) == FAV_OK && hipStreamSynchronize(nullptr) == hipSuccess;
    fav_status st = FAV_OK;
    if (!ok) { h->err = fmt("%s: cannot copy the bank to the device: %s", fn, hipGetErrorString(hipGetLastError())); st = FAV_ERR_HIP; }
    if (st == FAV_OK && h->patch_on) st = wait_enqueued(h);
    if (st != FAV_OK) { free_patch(&nw); return st; }
    if (h->patch_on) free_patch(&h->patch);
    h->patch = nw;
    h->patch_on = true;
    return FAV_OK;
}
// the tap the head reads, and its nouns; a stage mismatch is refused in front of the shared gate, naming both stages
bool patch_at_site(const fav_handle* h) { return h && h->patch_on && h->patch.stage > 0; }
fav_status patch_stage_gate(fav_handle* h, const char* fn) {
    if (!h) return FAV_OK;
    const std::string why = patch_stage_error(h);
    if (why.empty()) return FAV_OK;
    route_clear();
    h->err = fmt("%s: %s", fn, why.c_str());
    return FAV_ERR_INVALID_ARG;
}
}  // namespace

fav_status fav_set_patch_bank(fav_handle* h, const fav_patch_bank* b) { return set_patch_bank(h, b, nullptr, "fav_set_patch_bank"); }

fav_status fav_check_patch_site(const fav_patch_site* site, char* err, size_t err_cap) {
    static_assert(sizeof(fav_patch_site) == 12, "fav_patch_site is 3 dwords");
    return check_reply(patch_site_error(site), err, err_cap);
}

fav_status fav_set_patch_bank_at(fav_handle* h, const fav_patch_bank* b, const fav_patch_site* site) {
    return set_patch_bank(h, b, site, site ? "fav_set_patch_bank_at" : "fav_set_patch_bank");
}

fav_status fav_patch(fav_handle* h, float* dist, int32_t* row, fav_patch_record* rec, void* stream) {
    if (fav_status st = patch_stage_gate(h, "fav_patch")) return st;
    const bool at = patch_at_site(h);
    return map_head_on_last_call(h, "fav_patch", at ? kStageWords : kMapWords, at ? &fav_handle::stage_tap : &fav_handle::map_tap,
                                 bad_patch_buffers(dist, row, rec),
                                 [&] { return patch_handle_error(h); }, stream,
                                 [&](hipStream_t s) { return patch_on_tap(h, dist, row, rec, s); });
}

fav_status fav_classify_patch(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, int32_t* labels,
                              float* conf, uint8_t* fail, float* score, float* dist, int32_t* row, fav_patch_record* rec, void* stream) {
    if (fav_status st = patch_stage_gate(h, "fav_classify_patch")) return st;
    const bool at = patch_at_site(h);
    return classify_map_head(h, "fav_classify_patch", at ? kStageWords : kMapWords, at ? &fav_handle::stage_tap : &fav_handle::map_tap,
                             bad_patch_buffers(dist, row, rec),
                             [&] { return patch_handle_error(h); }, images, n, layout, first_index, labels, conf, fail, score, stream,
                             [&](hipStream_t s) { return patch_on_tap(h, dist, row, rec, s); });
}

// ---- deletion / insertion curves (fav_curve.hpp) --------------------------------
fav_status fav_check_curve(const fav_curve* desc, int32_t H, int32_t W, int32_t layout, char* err, size_t err_cap) {
    static_assert(sizeof(fav_curve) == 32, "fav_curve is 8 dwords");
    return check_reply(curve_desc_error(desc, H, W, layout), err, err_cap);
}

fav_status fav_set_curve(fav_handle* h, const fav_curve* desc) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!desc) return perturb_clear(h, h->curve, h->curve_on);
    const fav_status st = perturb_commit(
        h, "fav_set_curve", h->curve, h->curve_on, [&](int layout) { return curve_desc_error(desc, h->cfg.in_h, h->cfg.in_w, layout); },
        kCurveViews, [&](fav_handle::PerturbDev& d, std::string& what) {
            what = fmt("a curve of max_batch=%d frames and %d steps", (int)h->cfg.max_batch, desc->steps);
            std::vector<PerturbPart> parts = perturb_parts(h, d, desc->steps + 1);
            parts.push_back({(size_t)h->cfg.max_batch * CV_MAX_CELLS * 4, (void**)&d.rank});
            parts.push_back({parts[1].bytes, (void**)&d.lab});
            return parts;
        });
    if (st == FAV_OK) h->curve_desc = *desc;
    return st;
}

fav_status fav_classify_curve(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, const float* map,
                              int32_t mh, int32_t mw, const int32_t* classes, int32_t mode, int32_t* labels, float* conf, float* curve,
                              fav_curve_record* rec, void* stream) {
    static_assert(sizeof(fav_curve_record) == 32, "fav_curve_record is 8 dwords");
    const bool bad = !images || !map || !curve || !rec ||
                     (((uintptr_t)map | (uintptr_t)curve | (uintptr_t)classes | (uintptr_t)labels | (uintptr_t)conf) & 3) || ((uintptr_t)rec & 7);
    // every pass, the unoccluded one too, is classified from the occlusion buffer; its plane is its step
    auto pass = [&](int k, hipStream_t s) {
        const fav_handle::PerturbDev& cv = h->curve;
        const int S = h->curve_desc.steps, H = h->cfg.in_h, W = h->cfg.in_w;
        const int step = mode == FAV_CURVE_DELETION ? k : S - k;         // the unoccluded step first, then by increasing occlusion
        if (k == 0) launch_rank_cells(map, n, mh * mw, cv.rank, s);
        launch_occlude(images, cv.frames, cv.rank, n, H, W, layout, mh, mw, mode, S, step, step + 1,
                       layout == FAV_LAYOUT_NHWC_U8 ? h->curve_desc.fill_u8 : h->curve_desc.fill_f32_bits, s);
        return PerturbPass{cv.frames, cv.prob + (size_t)step * n, cv.lab + (size_t)step * n};
    };
    return classify_perturb_head(
        h, "fav_classify_curve", &fav_handle::curve_on, "no curve descriptor set (fav_set_curve)", &fav_handle::curve, bad, images, n, layout,
        first_index, classes, labels, conf, stream,
        [&] { const std::string why = curve_mode_error(mode); return why.empty() ? curve_map_error(mh, mw) : why; }, pass,
        [&](const int32_t* cls, hipStream_t s) {
            launch_curve(h->curve.prob, h->curve.lab, cls, n, h->curve_desc.steps, mh * mw, mode, h->cfg.num_classes, curve, rec, s);
        });
}

// ---- RISE saliency (fav_rise.hpp) ------------------------------------------------
fav_status fav_check_rise(const fav_rise* desc, int32_t H, int32_t W, int32_t layout, char* err, size_t err_cap) {
    static_assert(sizeof(fav_rise) == 48 && offsetof(fav_rise, seed) == 16 && offsetof(fav_rise, fill_u8) == 24, "fav_rise is 12 dwords");
    return check_reply(rise_desc_error(desc, H, W, layout), err, err_cap);
}

fav_status fav_set_rise(fav_handle* h, const fav_rise* desc) {
    if (!h) return FAV_ERR_INVALID_ARG;
    if (!desc) return perturb_clear(h, h->rise, h->rise_on);
    const fav_status st = perturb_commit(
        h, "fav_set_rise", h->rise, h->rise_on, [&](int layout) { return rise_desc_error(desc, h->cfg.in_h, h->cfg.in_w, layout); },
        kRiseViews, [&](fav_handle::PerturbDev& d, std::string& what) {
            what = fmt("RISE of max_batch=%d frames and %d masks", (int)h->cfg.max_batch, desc->n_masks);
            return perturb_parts(h, d, desc->n_masks + 1);
        });
    if (st == FAV_OK) h->rise_desc = *desc;
    return st;
}

fav_status fav_classify_rise(fav_handle* h, const void* images, int32_t n, int32_t layout, int64_t first_index, const int32_t* classes,
                             int32_t mh, int32_t mw, int32_t* labels, float* conf, float* map, fav_rise_record* rec, void* stream) {
    static_assert(sizeof(fav_rise_record) == 32, "fav_rise_record is 8 dwords");
    static_assert(offsetof(fav_rise_record, peak) == offsetof(fav_cam_record, peak) && offsetof(fav_rise_record, floor) == offsetof(fav_cam_record, floor),
                  "fav_op_cam_heatmap reads peak and floor of either record");
    const bool bad = !images || !map || !rec || (((uintptr_t)map | (uintptr_t)classes | (uintptr_t)labels | (uintptr_t)conf) & 3) ||
                     ((uintptr_t)rec & 7);
    // the unmasked pass is classified from the caller's frames; pass k > 0 is mask k - 1 and fills plane k
    auto pass = [&](int k, hipStream_t s) {
        const fav_handle::PerturbDev& rv = h->rise;
        if (k == 0) return PerturbPass{images, rv.prob, nullptr};
        launch_rise_mask(images, rv.frames, n, h->cfg.in_h, h->cfg.in_w, layout, h->rise_desc, first_index, k - 1, k, s);
        return PerturbPass{rv.frames, rv.prob + (size_t)k * n, nullptr};
    };
    return classify_perturb_head(
        h, "fav_classify_rise", &fav_handle::rise_on, "no RISE descriptor set (fav_set_rise)", &fav_handle::rise, bad, images, n, layout,
        first_index, classes, labels, conf, stream, [&] { return rise_map_error(mh, mw, h->cfg.in_h, h->cfg.in_w); }, pass,
        [&](const int32_t* cls, hipStream_t s) {
            launch_rise_accumulate(h->rise.prob, cls, n, h->rise_desc, first_index, h->cfg.in_h, h->cfg.in_w, mh, mw, h->cfg.num_classes, map,
                                   rec, s);
        });
}

fav_status fav_set_profiling(fav_handle* h, int32_t enable) {
    if (!h) return FAV_ERR_INVALID_ARG;
    h->profiling = enable != 0;
    h->ev_used = 0;
    memset(&h->prof, 0, sizeof h->prof);
    h->op_prof.assign(h->plan.ops.size(), fav_op_profile{});
    for (size_t i = 0; i < h->plan.ops.size(); ++i) {
        const Op& o = h->plan.ops[i];
        fav_op_profile& r = h->op_prof[i];
        r.op_index = (int)i; r.kind = (int)o.kind;
        r.H = o.H; r.W = o.W; r.Cin = o.C; r.Ho = o.Ho; r.Wo = o.Wo; r.Cout = o.Co;
        r.kh = r.kw = r.stride = 0;
        if (o.layer >= 0) { const LayerShape& L = h->plan.layers[o.layer]; r.kh = L.kh; r.kw = L.kw; r.stride = L.stride; }
        if (o.kind == OP_ENTRY_REDUCE) { r.reserved = o.Co2; r.kh = r.kw = r.stride = 1; r.Ho = o.H; r.Wo = o.W; r.Cout = o.C; }
        if (o.kind == OP_TAIL) { r.reserved = o.Co2; if (o.layer < 0) { r.kh = r.kw = r.stride = 1; } }   // reserved: channels of the fused next-block conv1
    }
    return FAV_OK;
}

fav_status fav_get_profile(fav_handle* h, fav_profile* out, int32_t reset) {
    if (!h || !out) return FAV_ERR_INVALID_ARG;
    HIP_TRY(h, hipDeviceSynchronize());
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b) == hipSuccess) {
            h->prof.ms[h->ev_pool[i].cls] += ms;
            const int op = h->ev_pool[i].op;
            if (op >= 0 && op < (int)h->op_prof.size()) h->op_prof[op].ms += ms;
        }
    }
    h->ev_used = 0;
    *out = h->prof;
    if (reset) memset(&h->prof, 0, sizeof h->prof);
    return FAV_OK;
}

fav_status fav_get_op_profile(fav_handle* h, fav_op_profile* out, int32_t cap, int32_t* n_out) {
    if (!h || !n_out) return FAV_ERR_INVALID_ARG;
    *n_out = (int32_t)h->op_prof.size();
    if (out) for (int i = 0; i < cap && i < (int)h->op_prof.size(); ++i) out[i] = h->op_prof[i];
    return FAV_OK;
}

// ---- operator level --------------------------------------------------------
static fav_status op_done(const char* e) {
    route_close(!e);
    if (e) { g_create_error = e; return FAV_ERR_INVALID_ARG; }
    if (hipGetLastError() != hipSuccess) { route_clear(); g_create_error = "kernel launch failed"; return FAV_ERR_HIP; }
    return FAV_OK;
}
// the same for a launcher's message ("conv: ..."), which does not name the entry point: "<fn>: conv: ..."
static fav_status op_done(const char* fn, const char* e) {
    route_close(!e);
    if (e) { g_create_error = fmt("%s: %s", fn, e); return FAV_ERR_INVALID_ARG; }
    if (hipGetLastError() != hipSuccess) { route_clear(); g_create_error = "kernel launch failed"; return FAV_ERR_HIP; }
    return FAV_OK;
}

fav_status fav_op_last_route(char* out, size_t cap) {
    if (!out || cap == 0) { g_create_error = "fav_op_last_route: null or empty buffer"; return FAV_ERR_INVALID_ARG; }
    const std::string t = route_text(g_route);
    if (t.size() + 1 > cap) {
        out[0] = 0;
        g_create_error = fmt("fav_op_last_route: the name needs %zu bytes, the buffer has %zu", t.size() + 1, cap);
        return FAV_ERR_INVALID_ARG;
    }
    memcpy(out, t.c_str(), t.size() + 1);
    return FAV_OK;
}

// the gates in front of a convolution's and a tail's selector: what fav_op_* and fav_route_* refuse alike
static const char* conv_gate(const fav_conv_desc* d) {
    if (!d || !d->x || !d->w || !d->bias || !d->y) return "null pointer";
    return d->Cout % 64 != 0 ? "Cout must be a multiple of 64" : nullptr;
}
static const char* tail_gate(const fav_tail_desc* d) {
    if (!d || !d->x || !d->wc || !d->bias_c || !d->res || !d->y) return "null pointer";
    return ((d->wb && !d->bias_b) || (d->wa && (!d->bias_a || !d->t1n))) ? "null pointer" : nullptr;
}

fav_status fav_op_conv2d(const fav_conv_desc* d, void* stream) {
    if (const char* e = conv_gate(d)) return op_done("fav_op_conv2d", e);
    return op_done("fav_op_conv2d", launch_conv(nullptr, *d, d->Cout, d->Cout, false, Group{}, (hipStream_t)stream));
}

fav_status fav_op_bottleneck_tail(const fav_tail_desc* d, void* stream) {
    if (const char* e = tail_gate(d)) return op_done("fav_op_bottleneck_tail", e);
    return op_done("fav_op_bottleneck_tail", launch_tail(nullptr, *d, Group{}, (hipStream_t)stream));
}

// ---- route queries: the selector's answer as text.  No device, no launch, and fav_op_last_route keeps what it had.
static fav_status route_reply(const char* gate, const Route& r, char* out, size_t cap) {
    const char* refusal = gate ? gate : r.refusal;
    const std::string t = refusal ? refusal : route_text(r);
    if (!out || t.size() + 1 > cap) return FAV_ERR_INVALID_ARG;
    memcpy(out, t.c_str(), t.size() + 1);
    return refusal ? FAV_ERR_INVALID_ARG : FAV_OK;
}

fav_status fav_route_conv2d(const fav_conv_desc* d, int32_t vit, int32_t groups, char* out, size_t cap) {
    const char* gate = groups < 1 ? "groups must be >= 1" : conv_gate(d);
    return route_reply(gate, gate ? Route{} : route_conv(*d, d->Cout, d->Cout, vit != 0, groups), out, cap);
}

fav_status fav_route_bottleneck_tail(const fav_tail_desc* d, int32_t groups, char* out, size_t cap) {
    const char* gate = groups < 1 ? "groups must be >= 1" : tail_gate(d);
    return route_reply(gate, gate ? Route{} : route_tail(*d, groups), out, cap);
}

fav_status fav_route_attention(int32_t n, int32_t T, int32_t D, int32_t heads, int32_t math_mode, char* out, size_t cap) {
    return route_reply(nullptr, route_attention(n, T, D, heads, math_mode), out, cap);
}

fav_status fav_op_stem_im2col(const void* images, int32_t layout, int32_t n, int32_t H, int32_t W, int32_t kh, int32_t kw,
                              int32_t stride, int32_t pad, int32_t kpad, const float* mean3, const float* inv_std3,
                              void* out, void* stream) {
    if (!images || !out || !mean3 || !inv_std3 || kpad % 64 != 0 || kpad < kh * kw * 3) return op_done("fav_op_stem_im2col: bad argument");
    return op_done("fav_op_stem_im2col", launch_stem(nullptr, images, layout, n, H, W, kh, kw, stride, pad, kpad, mean3, inv_std3, out, (hipStream_t)stream));
}

fav_status fav_op_stem_pool(const void* images, int32_t layout, int32_t n, int32_t H, int32_t W, const void* w, const float* bias,
                            const float* mean3, const float* inv_std3, void* out, void* stream) {
    if (!images || !w || !bias || !mean3 || !inv_std3 || !out) return op_done("fav_op_stem_pool: null argument");
    return op_done(launch_stem_pool(nullptr, images, layout, n, H, W, w, bias, mean3, inv_std3, out, Group{}, (hipStream_t)stream));
}

fav_status fav_op_maxpool3x3s2(const void* x, void* y, int32_t n, int32_t H, int32_t W, int32_t C, void* stream) {
    if (!x || !y || C % 8 != 0) return op_done("fav_op_maxpool3x3s2: bad argument");
    return op_done("fav_op_maxpool3x3s2", launch_maxpool(nullptr, x, y, n, H, W, C, (hipStream_t)stream));
}

fav_status fav_op_avgpool(const void* x, void* y, int32_t n, int32_t HW, int32_t C, const fav_dropout_desc* drop, void* stream) {
    if (!x || !y || C % 16 != 0) return op_done("fav_op_avgpool: bad argument");
    return op_done("fav_op_avgpool", launch_avgpool(nullptr, x, y, n, HW, C, drop, Group{}, (hipStream_t)stream));
}

fav_status fav_op_entry_reduce(const void* x, void* y, const void* wa, const float* bias_a, void* t1, int32_t C, int32_t Nred,
                               int32_t HW, int32_t n_out, const fav_dropout_desc* drop, void* stream) {
    if (!x || !wa || !bias_a || !t1) return op_done("fav_op_entry_reduce: bad argument");
    return op_done("fav_op_entry_reduce", launch_entry_reduce(nullptr, x, y, wa, bias_a, t1, C, Nred, HW, n_out, drop, (hipStream_t)stream));
}

fav_status fav_op_entry_dropout(const void* x, void* out, int64_t elems, int32_t n_out, const fav_dropout_desc* drop, void* stream) {
    if (!x || !out || elems % 16 != 0) return op_done("fav_op_entry_dropout: bad argument");
    return op_done("fav_op_entry_dropout", launch_entry_dropout(nullptr, x, out, elems, n_out, drop, (hipStream_t)stream));
}

fav_status fav_op_head(const float* logits, int32_t T, int32_t n, int32_t C, int32_t ld, float temperature, int32_t kind,
                       float tau, int32_t* labels, float* conf, uint8_t* fail, float* score, void* stream) {
    if (!logits || !labels || !conf || T < 1 || n < 1 || !(temperature > 0.f)) return op_done("fav_op_head: bad argument");
    if (kind == FAV_CONF_MUTUAL_INFO && (T < 2 || C < 2))
        return op_done("fav_op_head: conf_kind 2 (mutual information) needs T >= 2 samples and num_classes >= 2");
    HeadOut out;
    out.labels = labels; out.conf = conf; out.fail = fail; out.score = score;
    return op_done(launch_head(nullptr, logits, T, n, C, ld, temperature, kind, tau, out, (hipStream_t)stream));
}

fav_status fav_op_head_uncertainty(const float* logits, int32_t T, int32_t n, int32_t C, int32_t ld, float temperature,
                                   int32_t kind, float tau, fav_uncertainty* records, uint8_t* fail, float* score, void* stream) {
    if (!logits || !records || ((uintptr_t)records & 7) || T < 1 || T > 4096 || n < 1 || kind < 0 || kind > 2 ||
        !(temperature > 0.f))
        return op_done("fav_op_head_uncertainty: bad argument (records non-NULL and 8-byte aligned, 1 <= T <= 4096, kind 0..2)");
    HeadOut out;
    out.rec = records; out.fail = fail; out.score = score;
    return op_done(launch_head(nullptr, logits, T, n, C, ld, temperature, kind, tau, out, (hipStream_t)stream));
}

fav_status fav_op_head_sets(const float* logits, int32_t T, int32_t n, int32_t C, int32_t ld, float temperature, int32_t kind,
                            float tau, int64_t first_index, const fav_conformal* cp, const int32_t* true_labels,
                            float* true_scores, fav_pred_set* records, uint8_t* fail, float* score, void* stream) {
    if (!logits || T < 1 || n < 1 || kind < 0 || kind > 2 || !(temperature > 0.f))
        return op_done("fav_op_head_sets: bad argument (logits non-NULL, T >= 1, n >= 1, kind 0..2, temperature > 0)");
    const HeadSets hs{cp, first_index, true_labels, true_scores, records};
    HeadOut out;
    out.sets = &hs; out.fail = fail; out.score = score;
    return op_done(launch_head(nullptr, logits, T, n, C, ld, temperature, kind, tau, out, (hipStream_t)stream));
}

fav_status fav_op_head_sweep(const float* logits, int32_t T, int32_t n, int32_t C, int32_t ld, const float* temps, int32_t K,
                             int32_t kind, const int32_t* true_labels, fav_calib_cell* cells, void* stream) {
    const HeadSweep sw{temps, K, true_labels, cells};
    if (const char* e = check_sweep(sw, C, T, kind)) return op_done(fmt("fav_op_head_sweep: %s", e).c_str());
    if (!logits || T < 1 || n < 1) return op_done("fav_op_head_sweep: bad argument (logits non-NULL, T >= 1, n >= 1)");
    HeadOut out;
    out.sweep = &sw;
    return op_done(launch_head(nullptr, logits, T, n, C, ld, 1.0f, kind, 0.f, out, (hipStream_t)stream));
}

fav_status fav_op_layernorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t rows, int32_t D,
                            float eps, void* stream) {
    if (!x || !gamma || !beta || !y) return op_done("fav_op_layernorm: null pointer");
    return op_done(launch_layernorm(nullptr, x, ldx, gamma, beta, y, rows, D, eps, (hipStream_t)stream));
}

fav_status fav_op_attention(const void* qkv, void* out, int32_t n, int32_t T, int32_t D, int32_t heads, int32_t math_mode,
                            void* stream) {
    if (!qkv || !out) return op_done("fav_op_attention: null pointer");
    return op_done(launch_attention(nullptr, qkv, out, n, T, D, heads, math_mode, (hipStream_t)stream));
}

fav_status fav_op_linear_streamk(const fav_linear_desc* d, void* stream) {
    if (!d || !d->x || !d->w || !d->bias || !d->y) return op_done("fav_op_linear_streamk: null pointer");
    if (!launch_gemm_streamk(nullptr, d->x, d->w, d->bias, d->res, d->y, d->rows, d->K, d->N, d->act, (hipStream_t)stream))
        return op_done("fav_op_linear_streamk: shape not supported (K % 32, N % 128, >= 256 tiles of 128 x 128, 32-bit offsets)");
    return op_done(nullptr);
}

fav_status fav_op_vit_assemble(const void* emb, const float* pos, void* x, int32_t n, int32_t ntok, int32_t D, void* stream) {
    if (!emb || !pos || !x || n < 1 || ntok < 2 || D % 4 != 0) return op_done("fav_op_vit_assemble: bad argument");
    launch_vit_assemble(nullptr, emb, pos, x, n, ntok, D, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_signal_stats(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const uint8_t* prev_gray,
                               uint8_t* last_gray, fav_signal_stats* stats, void* stream) {
    static_assert(sizeof(fav_signal_stats) == sizeof(SignalStats), "fav_signal_stats layout");
    if (!frames || !stats || n < 1 || H < 3 || W < 4 || W % 4 != 0 || (long long)H * W > 150000)
        return op_done("fav_op_signal_stats: bad argument (need W % 4 == 0, 3 <= H, H*W <= 150000)");
    // the kernel reads frames and prev_gray, and writes last_gray, four pixels a dword; the records hold doubles
    if (((uintptr_t)frames | (uintptr_t)prev_gray | (uintptr_t)last_gray) % 4 != 0 || (uintptr_t)stats % 8 != 0)
        return op_done("fav_op_signal_stats: frames, prev_gray and last_gray must be 4-byte aligned, stats 8-byte aligned");
    const size_t lds = (((size_t)H * W + 15) & ~(size_t)15) + 1024 * 4 + 16 * 8;
    if (hipFuncSetAttribute((const void*)signal_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return op_done("fav_op_signal_stats: cannot reserve LDS for the gray plane");
    hipLaunchKernelGGL(signal_stats_kernel, dim3(n), dim3(256), lds, (hipStream_t)stream, frames, n, H, W, prev_gray,
                       last_gray, (SignalStats*)stats);
    return op_done(nullptr);
}

fav_status fav_op_corrupt(const uint8_t* frames, void* out, int32_t n, int32_t H, int32_t W, int32_t mode, float level,
                          float gain, float sigma, uint64_t seed, int64_t first_index, void* stream) {
    if (!frames || !out || n < 1 || H < 1 || W < 1 || mode < 0 || mode > 3) return op_done("fav_op_corrupt: bad argument");
    CorruptParams cp;
    cp.mode = mode; cp.level = level; cp.gain = gain; cp.sigma = sigma;
    cp.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull); cp.seed_hi = (uint32_t)(seed >> 32); cp.first_index = first_index;
    hipLaunchKernelGGL(corrupt_kernel, dim3(grid_for((long long)n * H * W)), dim3(256), 0, (hipStream_t)stream, frames, out,
                       n, H, W, cp);
    return op_done(nullptr);
}

// ---- the ImageNet-C style corruption family (fav_corrupt_c.hpp)
static const float kCorruptionSeverity[FAV_C_COUNT][5][2] = {
    {{.03f, 0.f}, {.06f, 0.f}, {.09f, 0.f}, {.17f, 0.f}, {.27f, 0.f}},      // impulse: amount
    {{.15f, 0.f}, {.2f, 0.f}, {.35f, 0.f}, {.45f, 0.f}, {.6f, 0.f}},        // speckle: sigma
    {{1.f, 0.f}, {2.f, 0.f}, {3.f, 0.f}, {4.f, 0.f}, {6.f, 0.f}},           // gaussian blur: sigma
    {{3.f, .1f}, {4.f, .5f}, {6.f, .5f}, {8.f, .5f}, {10.f, .5f}},          // defocus: radius, alias sigma
    {{.4f, 0.f}, {.3f, 0.f}, {.2f, 0.f}, {.1f, 0.f}, {.05f, 0.f}},          // contrast: c
    {{.6f, 0.f}, {.5f, 0.f}, {.4f, 0.f}, {.3f, 0.f}, {.25f, 0.f}},          // pixelate: c
    {{.1f, 0.f}, {.2f, 0.f}, {.3f, 0.f}, {.4f, 0.f}, {.5f, 0.f}},           // brightness: c
    {{.3f, 0.f}, {.1f, 0.f}, {2.f, 0.f}, {5.f, .1f}, {20.f, .2f}},          // saturate: a, b
};

// what is wrong with (kind, a, b), or nullptr
static const char* corruption_params_error(int32_t kind, float a, float b) {
    if (kind < 0 || kind >= FAV_C_COUNT) return "kind outside [0, FAV_C_COUNT)";
    if (!std::isfinite(a) || !std::isfinite(b)) return "a and b must be finite";
    switch (kind) {
    case FAV_C_IMPULSE_NOISE: return a >= 0.f && a <= 1.f ? nullptr : "impulse amount a outside [0, 1]";
    case FAV_C_SPECKLE_NOISE: return a >= 0.f ? nullptr : "speckle sigma a below 0";
    case FAV_C_GAUSSIAN_BLUR:
        if (!(a > 0.f)) return "gaussian blur sigma a must be above 0";
        return 4.0 * (double)a + 0.5 < (double)(CC_GAUSS_MAX_R + 1) ? nullptr : "gaussian blur radius (int)(4 a + 0.5) above 32";
    case FAV_C_DEFOCUS_BLUR:
        if (!(a >= 1.f && a < 13.f)) return "defocus radius (int)a outside 1..12";
        return b > 0.f ? nullptr : "defocus alias sigma b must be above 0";
    case FAV_C_CONTRAST: return a >= 0.f && a <= 1.f ? nullptr : "contrast a outside [0, 1]";
    case FAV_C_PIXELATE: return a > 0.f && a <= 1.f ? nullptr : "pixelate a outside (0, 1]";
    case FAV_C_BRIGHTNESS: return a >= 0.f && a <= 1.f ? nullptr : "brightness a outside [0, 1]";
    default:
        if (!(a >= 0.f)) return "saturate a below 0";
        return b >= -1.f && b <= 1.f ? nullptr : "saturate b outside [-1, 1]";
    }
}

// EXPERIMENTS build only: FAV_CORRUPT_C_STORE = 1 / 2 stores a group's values straight from registers (float4 / scalar), read at
// every call so that one process can alternate; the normal build always stages a wave's stores through LDS
static int corrupt_c_store_mode() {
    const char* v = fav_knob_str("FAV_CORRUPT_C_STORE");
    return v ? std::max(0, std::min(2, atoi(v))) : CC_STORE_STAGED;
}

// an operator that refuses its arguments, before anything is launched
static fav_status op_rejected(const char* fn, const char* why) {
    g_create_error = fmt("%s: %s", fn, why);
    return FAV_ERR_INVALID_ARG;
}
// What an op that streams n frames in and n * count frames out (fav_op_views, fav_op_occlude, fav_op_rise_mask) refuses once
// its own parameters are in range: frames of another alignment than their elements', `own` (the op's complaint that stands in
// between; NULL: none), n * count (`span` in the message) beyond 31 bits, out overlapping frames.  "": nothing.
static std::string stream_out_error(const void* frames, const void* out, int n, int H, int W, int layout, int count, const char* span,
                                    const char* own) {
    const size_t esz = layout == FAV_LAYOUT_NHWC_U8 ? 1 : 4;
    if (((uintptr_t)frames | (uintptr_t)out) % esz != 0) return "fp32 frames and out must be 4-byte aligned";
    if (own) return own;
    if ((long long)n * count > 0x7FFFFFFFll) return fmt("n * %s above 2^31 - 1", span);
    const long long frame_bytes = (long long)H * W * 3 * (long long)esz;
    const uintptr_t in_lo = (uintptr_t)frames, in_hi = in_lo + (uintptr_t)frame_bytes * (uintptr_t)n;
    const uintptr_t out_lo = (uintptr_t)out, out_hi = out_lo + (uintptr_t)frame_bytes * (uintptr_t)n * (uintptr_t)count;
    return in_lo < out_hi && out_lo < in_hi ? "out overlaps frames" : "";
}

// The gate in front of a scoring head's launch: what fav_op_ood_score and fav_op_knn_score refuse alike, in the order both
// report it, or "".  dims: the head's *_dims_error; own(): the checks only that head has, which stand in front of the records'.
extern "C++" {   // a template
template <class Own>
static std::string score_gate(int S, int max_S, int n, const std::string& dims, float threshold, const void* records, Own own) {
    if (S < 1 || S > max_S) return fmt("S=%d outside [1, %d]", S, max_S);
    if (n < 1) return "n must be at least 1";
    if (!dims.empty()) return dims;
    if (std::isnan(threshold)) return "threshold is NaN";
    const std::string why = own();
    if (!why.empty()) return why;
    return (uintptr_t)records & 7 ? "records_dev must be 8-byte aligned" : "";
}
}  // extern "C++"

fav_status fav_corruption_params(int32_t kind, int32_t severity, float* a, float* b) {
    if (!a || !b) return op_rejected("fav_corruption_params", "null pointer");
    if (kind < 0 || kind >= FAV_C_COUNT) return op_rejected("fav_corruption_params", "kind outside [0, FAV_C_COUNT)");
    if (severity < 1 || severity > 5) return op_rejected("fav_corruption_params", "severity outside 1..5");
    *a = kCorruptionSeverity[kind][severity - 1][0];
    *b = kCorruptionSeverity[kind][severity - 1][1];
    return FAV_OK;
}

fav_status fav_corruption_taps(int32_t kind, float a, float b, float* taps, int32_t cap, int32_t* radius) {
    if (!taps || !radius) return op_rejected("fav_corruption_taps", "null pointer");
    if (kind != FAV_C_GAUSSIAN_BLUR && kind != FAV_C_DEFOCUS_BLUR)
        return op_rejected("fav_corruption_taps", "only the two blur kinds have taps");
    if (const char* why = corruption_params_error(kind, a, b)) return op_rejected("fav_corruption_taps", why);
    const int R = kind == FAV_C_GAUSSIAN_BLUR ? gauss_radius(a) : disk_radius(a);
    const int count = kind == FAV_C_GAUSSIAN_BLUR ? 2 * R + 1 : (2 * R + 1) * (2 * R + 1);
    if (cap < count) return op_rejected("fav_corruption_taps", "cap is smaller than the number of taps");
    if (kind == FAV_C_GAUSSIAN_BLUR) gauss_taps(a, R, taps);
    else disk_taps(a, b, taps);
    *radius = R;
    return FAV_OK;
}

fav_status fav_op_corrupt_c(const uint8_t* frames, float* out, int32_t n, int32_t H, int32_t W, const fav_corruption_desc* d,
                            void* stream) {
    static_assert(sizeof(fav_corruption_desc) == 32, "fav_corruption_desc layout");
    const char* fn = "fav_op_corrupt_c";
    route_clear();
    if (!frames || !out || !d) return op_rejected(fn, "null pointer");
    if (n < 1 || H < 1 || W < 1) return op_rejected(fn, "n, H and W must be at least 1");
    if (d->struct_size != sizeof(fav_corruption_desc)) return op_rejected(fn, "struct_size is not sizeof(fav_corruption_desc)");
    if (const char* why = corruption_params_error(d->kind, d->a, d->b)) return op_rejected(fn, why);
    if ((uintptr_t)out % 4 != 0) return op_rejected(fn, "out must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long npx = (long long)H * W, total = npx * n;
    const long long max_grid = (1ll << 24) - 1;
    CorruptCParams cp;
    cp.a = d->a; cp.b = d->b;
    cp.seed_lo = (uint32_t)(d->seed & 0xFFFFFFFFull); cp.seed_hi = (uint32_t)(d->seed >> 32); cp.first_index = d->first_frame_index;
    const int tiles_x = (W + CC_TILE - 1) / CC_TILE, tiles_y = (H + CC_TILE - 1) / CC_TILE;
    const long long tiles = (long long)tiles_x * tiles_y * n;
    const unsigned tile_grid = (unsigned)std::min(tiles, max_grid);
    switch (d->kind) {
    case FAV_C_IMPULSE_NOISE: case FAV_C_SPECKLE_NOISE: case FAV_C_BRIGHTNESS: case FAV_C_SATURATE: {
        const dim3 grid(grid_for(px_group_count(total)));
        const int store_mode = corrupt_c_store_mode();
        if (d->kind == FAV_C_IMPULSE_NOISE)
            hipLaunchKernelGGL((corrupt_c_point_kernel<CC_IMPULSE>), grid, dim3(256), 0, s, frames, out, npx, total, cp, store_mode);
        else if (d->kind == FAV_C_SPECKLE_NOISE)
            hipLaunchKernelGGL((corrupt_c_point_kernel<CC_SPECKLE>), grid, dim3(256), 0, s, frames, out, npx, total, cp, store_mode);
        else if (d->kind == FAV_C_BRIGHTNESS)
            hipLaunchKernelGGL((corrupt_c_point_kernel<CC_BRIGHTNESS>), grid, dim3(256), 0, s, frames, out, npx, total, cp, store_mode);
        else
            hipLaunchKernelGGL((corrupt_c_point_kernel<CC_SATURATE>), grid, dim3(256), 0, s, frames, out, npx, total, cp, store_mode);
        break;
    }
    case FAV_C_CONTRAST: {
        // blocks per frame: one per 4096 pixels, at most 16 (each of them reads the whole frame once for the sums)
        const int per_frame = (int)std::max<long long>(1, std::min<long long>((npx + 4095) / 4096, 16));
        if ((long long)n * per_frame > 0x7FFFFFFFll) return op_rejected(fn, "too many frames for one contrast launch");
        hipLaunchKernelGGL(contrast_kernel, dim3((unsigned)(n * per_frame)), dim3(256), 0, s, frames, out, npx, per_frame,
                           (double)H * W * 255.0, d->a, corrupt_c_store_mode());
        break;
    }
    case FAV_C_PIXELATE: {
        if (W > CC_PIXELATE_MAX_W) return op_rejected(fn, "pixelate takes frames up to 2048 pixels wide");
        const int hd = std::max(1, (int)((double)H * (double)d->a)), wd = std::max(1, (int)((double)W * (double)d->a));
        const long long items = (long long)n * hd;
        const size_t lds = (size_t)4 * W * 4 + (size_t)3 * wd * 4;
        hipLaunchKernelGGL(pixelate_kernel, dim3((unsigned)std::min(items, max_grid)), dim3(256), lds, s, frames, out, H, W, hd,
                           wd, items);
        break;
    }
    case FAV_C_GAUSSIAN_BLUR: {
        const int R = gauss_radius(d->a);
        GaussTaps tp;
        memset(&tp, 0, sizeof tp);
        gauss_taps(d->a, R, tp.v);
        hipLaunchKernelGGL(gauss_blur_kernel, dim3(tile_grid), dim3(256), gauss_blur_lds(R), s, frames, out, H, W, R, tp, tiles_x,
                           tiles_y, tiles);
        break;
    }
    default: {
        const int R = disk_radius(d->a);
        DiskTaps tp;
        memset(&tp, 0, sizeof tp);
        disk_taps(d->a, d->b, tp.v);
        hipLaunchKernelGGL(defocus_kernel, dim3(tile_grid), dim3(256), defocus_lds(R), s, frames, out, H, W, R, tp, tiles_x, tiles_y,
                           tiles);
        break;
    }
    }
    return op_done(nullptr);
}

fav_status fav_op_views(const void* frames, void* out, int32_t n, int32_t H, int32_t W, int32_t layout, const fav_view* views,
                        int32_t n_views, void* stream) {
    const char* fn = "fav_op_views";
    route_clear();
    if (!frames || !out) return op_rejected(fn, "null pointer");
    if (n < 1 || H < 1 || W < 1) return op_rejected(fn, "n, H and W must be at least 1");
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return op_rejected(fn, "unknown layout");
    std::string why = views_error(views, n_views, H, W);
    // the kernels hold a frame's work items in 32 bits: H * (1 + ceil(W / 4)) <= H * W / 4 + 2 H stays below 2^31
    if (why.empty())
        why = stream_out_error(frames, out, n, H, W, layout, n_views, "n_views",
                               (long long)H * W > 0x7FFFFFFFll / 12 ? "H * W above (2^31 - 1) / 12 pixels" : nullptr);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    launch_views(frames, out, n, H, W, layout, views, n_views, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_ood_score(const void* feat, int32_t S, int32_t n, int32_t D, int32_t k, int32_t R, const float* mu, const float* Pt,
                            const float* Mt, const int32_t* class_id, const int32_t* labels, float threshold,
                            fav_ood_record* records, void* stream) {
    const char* fn = "fav_op_ood_score";
    route_clear();
    if (!feat || !mu || !Pt || !Mt || !class_id || !records) return op_rejected(fn, "null pointer");
    const std::string why = score_gate(S, OOD_MAX_S, n, ood_dims_error(D, k, R), threshold, records, [] { return std::string(); });
    if (!why.empty()) return op_rejected(fn, why.c_str());
    launch_ood(feat, S, n, D, k, R, mu, Pt, Mt, class_id, labels, threshold, records, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_knn_score(const void* feat, int32_t S, int32_t n, int32_t D, const void* bank, int32_t N, int32_t k,
                            const int32_t* class_id, float threshold, void* ws, size_t ws_bytes, fav_knn_record* records,
                            void* stream) {
    const char* fn = "fav_op_knn_score";
    route_clear();
    if (!feat || !bank || !ws || !records) return op_rejected(fn, "null pointer");
    KnnWs w;
    const std::string why = score_gate(S, KNN_MAX_S, n, knn_dims_error(D, N, k), threshold, records, [&]() -> std::string {
        w = knn_workspace(n, D, N, false);
        if (ws_bytes < w.bytes) return fmt("ws_bytes=%zu is below fav_knn_workspace_bytes=%zu", ws_bytes, w.bytes);
        if ((uintptr_t)ws & 255) return "ws_dev must be 256-byte aligned";
        return (uintptr_t)bank & 15 ? "bank_dev must be 16-byte aligned" : "";
    });
    if (!why.empty()) return op_rejected(fn, why.c_str());
    hipStream_t s = (hipStream_t)stream;
    if (knn_prepare(w, ws, bank, D, N, false, s) != FAV_OK) { g_create_error = fmt("%s: cannot prepare the workspace: %s", fn, hipGetErrorString(hipGetLastError())); return FAV_ERR_HIP; }
    return op_done(fn, launch_knn(feat, S, n, D, bank, N, k, class_id, threshold, w, ws, false, records, s));
}

namespace {
// fav_op_patch_score (radius -1: the k-NN head's query kernel) and fav_op_patch_score_at (radius checked by the caller)
fav_status op_patch_score(const char* fn, const void* maps, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, const void* bank,
                          int32_t N, int32_t chunk_rows, float threshold, int radius, void* ws, size_t ws_bytes, float* dist,
                          int32_t* row, fav_patch_record* rec, void* stream) {
    route_clear();
    if (!maps || !bank || !ws || !dist || !rec) return op_rejected(fn, "null pointer");
    PatchWs w;
    std::string dims = patch_map_error(n, Hf, Wf);
    if (dims.empty()) dims = knn_dims_error(C, N, 1);
    if (dims.empty()) dims = patch_chunk_error(chunk_rows);
    const std::string why = score_gate(S, KNN_MAX_S, n, dims, threshold, rec, [&]() -> std::string {
        w = patch_workspace((long long)n * Hf * Wf, C, N, chunk_rows, false);
        if (ws_bytes < w.bytes) return fmt("ws_bytes=%zu is below fav_patch_workspace_bytes=%zu", ws_bytes, w.bytes);
        if ((uintptr_t)ws & 255) return "ws_dev must be 256-byte aligned";
        if (((uintptr_t)dist | (uintptr_t)row) & 3) return "dist_dev and row_dev must be 4-byte aligned";
        return (uintptr_t)bank & 15 ? "bank_dev must be 16-byte aligned" : "";
    });
    if (!why.empty()) return op_rejected(fn, why.c_str());
    hipStream_t s = (hipStream_t)stream;
    if (patch_prepare(w, ws, bank, C, N, false, s) != FAV_OK) { g_create_error = fmt("%s: cannot prepare the workspace: %s", fn, hipGetErrorString(hipGetLastError())); return FAV_ERR_HIP; }
    return op_done(fn, launch_patch(maps, S, n, Hf, Wf, C, radius, bank, N, threshold, w, ws, false, dist, row, rec, s));
}
}  // namespace

fav_status fav_op_patch_score(const void* maps, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, const void* bank, int32_t N,
                              int32_t chunk_rows, float threshold, void* ws, size_t ws_bytes, float* dist, int32_t* row,
                              fav_patch_record* rec, void* stream) {
    return op_patch_score("fav_op_patch_score", maps, S, n, Hf, Wf, C, bank, N, chunk_rows, threshold, -1, ws, ws_bytes, dist, row, rec, stream);
}

fav_status fav_op_patch_score_at(const void* maps, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, const void* bank, int32_t N,
                                 int32_t chunk_rows, float threshold, int32_t radius, void* ws, size_t ws_bytes, float* dist,
                                 int32_t* row, fav_patch_record* rec, void* stream) {
    const char* fn = "fav_op_patch_score_at";
    const std::string why = patch_radius_error(radius);
    if (!why.empty()) { route_clear(); return op_rejected(fn, why.c_str()); }
    if ((uintptr_t)maps & 15) { route_clear(); return op_rejected(fn, "maps_bf16 must be 16-byte aligned"); }
    return op_patch_score(fn, maps, S, n, Hf, Wf, C, bank, N, chunk_rows, threshold, radius, ws, ws_bytes, dist, row, rec, stream);
}

fav_status fav_op_patch_query(const void* maps, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, int32_t radius, void* q,
                              int32_t* flags, void* stream) {
    const char* fn = "fav_op_patch_query";
    route_clear();
    if (!maps || !q || !flags) return op_rejected(fn, "null pointer");
    const std::string why = patch_query_error(S, n, Hf, Wf, C, radius);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)maps | (uintptr_t)q) & 15) return op_rejected(fn, "maps_bf16 and q_dev must be 16-byte aligned");
    if ((uintptr_t)flags & 3) return op_rejected(fn, "flags_dev must be 4-byte aligned");
    launch_patch_query(maps, S, n, Hf, Wf, C, radius, q, flags, (hipStream_t)stream);
    return op_done(nullptr);
}

// ---- greedy coreset selection (fav_coreset.hpp) ----------------------------------
fav_status fav_check_coreset(int32_t N, int32_t D, int32_t M, int32_t start_row, char* err, size_t err_cap) {
    return check_reply(coreset_error(N, D, M, start_row), err, err_cap);
}

size_t fav_coreset_workspace_bytes(int32_t N, int32_t D, int32_t M) {
    if (!coreset_error(N, D, M, 0).empty()) return 0;
    return coreset_workspace(N).bytes;
}

fav_status fav_op_coreset_select(const void* rows, int32_t N, int32_t D, int32_t M, int32_t start_row, void* ws, size_t ws_bytes,
                                 int32_t* order, float* radius, void* stream) {
    const char* fn = "fav_op_coreset_select";
    route_clear();
    if (!rows || !ws || !order || !radius) return op_rejected(fn, "null pointer");
    const std::string dims = coreset_error(N, D, M, start_row);
    if (!dims.empty()) return op_rejected(fn, dims.c_str());
    const size_t need = coreset_workspace(N).bytes;
    if (ws_bytes < need) return op_rejected(fn, fmt("ws_bytes=%zu is below fav_coreset_workspace_bytes=%zu", ws_bytes, need).c_str());
    if ((uintptr_t)ws & 255) return op_rejected(fn, "ws_dev must be 256-byte aligned");
    if (((uintptr_t)rows | (uintptr_t)order | (uintptr_t)radius) & 15) return op_rejected(fn, "rows_bf16_dev, order_dev and radius_dev must be 16-byte aligned");
    launch_coreset(rows, N, D, M, start_row, ws, order, radius, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_drift_test(const void* feat, int32_t S, int32_t n, int32_t D, const void* ref, int32_t R, int32_t n_perm,
                             uint64_t seed, float alpha, void* ws, size_t ws_bytes, fav_drift_record* record, int64_t* perm_sums,
                             void* stream) {
    const char* fn = "fav_op_drift_test";
    route_clear();
    if (!feat || !ref || !ws || !record) return op_rejected(fn, "null pointer");
    DriftWs w;
    const std::string why = score_gate(S, DRIFT_MAX_S, n, drift_dims_error(D, R, n_perm, alpha, &n), 0.f, record, [&]() -> std::string {
        w = drift_workspace(n, D, R, n_perm, false);
        if (ws_bytes < w.bytes) return fmt("ws_bytes=%zu is below fav_drift_workspace_bytes=%zu", ws_bytes, w.bytes);
        if ((uintptr_t)ws & 255) return "ws_dev must be 256-byte aligned";
        if ((uintptr_t)perm_sums & 7) return "perm_sums_dev must be 8-byte aligned";
        return (uintptr_t)ref & 15 ? "ref_dev must be 16-byte aligned" : "";
    });
    if (!why.empty()) return op_rejected(fn, why.c_str());
    hipStream_t s = (hipStream_t)stream;
    // the pool: the reference at the front, zero rows behind the window's; and the zero bias
    const size_t row = (size_t)D * 2, Np = (size_t)R + n;
    char* const pool = (char*)ws + w.pool;
    if (hipMemcpyAsync(pool, ref, R * row, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        ((size_t)w.ld > Np && hipMemsetAsync(pool + Np * row, 0, ((size_t)w.ld - Np) * row, s) != hipSuccess) ||
        hipMemsetAsync((char*)ws + w.bias, 0, (size_t)w.ld * 4, s) != hipSuccess) {
        g_create_error = fmt("%s: cannot prepare the workspace: %s", fn, hipGetErrorString(hipGetLastError()));
        return FAV_ERR_HIP;
    }
    return op_done(fn, launch_drift(feat, S, n, D, R, n_perm, seed, alpha, w, ws, false, record, perm_sums, s));
}

fav_status fav_op_cam(const void* maps, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, const void* w, int32_t ldw,
                      const float* bias, int32_t n_classes, const int32_t* classes, int32_t K, float* cam, fav_cam_record* rec,
                      void* stream) {
    const char* fn = "fav_op_cam";
    route_clear();
    if (!maps || !w || !bias || !classes || !cam || !rec) return op_rejected(fn, "null pointer");
    const std::string why = cam_dims_error(S, n, Hf, Wf, C, ldw, n_classes, K);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)maps | (uintptr_t)w) & 15) return op_rejected(fn, "maps_bf16 and w_bf16 must be 16-byte aligned");
    if (((uintptr_t)bias | (uintptr_t)classes | (uintptr_t)cam) & 3) return op_rejected(fn, "bias, classes_dev and cam_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    return op_done(fn, launch_cam(maps, S, n, Hf, Wf, C, w, ldw, bias, n_classes, classes, K, cam, rec, (hipStream_t)stream));
}

fav_status fav_op_cam_heatmap(const float* cam, const fav_cam_record* rec, int32_t m, int32_t Hf, int32_t Wf, int32_t H, int32_t W,
                              uint8_t* out, void* stream) {
    const char* fn = "fav_op_cam_heatmap";
    route_clear();
    if (!cam || !rec || !out) return op_rejected(fn, "null pointer");
    const std::string why = cam_heatmap_dims_error(m, Hf, Wf, H, W);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if ((uintptr_t)cam & 3) return op_rejected(fn, "cam_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    launch_cam_heatmap(cam, rec, m, Hf, Wf, H, W, out, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_attn_mean(const void* qkv, float* a, int32_t n, int32_t T, int32_t D, int32_t heads, void* stream) {
    const char* fn = "fav_op_attn_mean";
    route_clear();
    if (!qkv || !a) return op_rejected(fn, "null pointer");
    const std::string why = attn_mean_dims_error(n, T, D, heads);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)qkv | (uintptr_t)a) & 15) return op_rejected(fn, "qkv_bf16 and a_dev must be 16-byte aligned");
    launch_attn_mean(qkv, a, n, T, D, heads, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_attn_rollout(const float* a, int32_t L, int32_t n, int32_t gh, int32_t gw, int32_t ld, int32_t first_layer, float* map,
                               fav_rollout_record* rec, void* stream) {
    const char* fn = "fav_op_attn_rollout";
    route_clear();
    if (!a || !map || !rec) return op_rejected(fn, "null pointer");
    const std::string why = rollout_dims_error(L, n, gh, gw, ld, first_layer);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)a | (uintptr_t)map) & 3) return op_rejected(fn, "a_dev and map_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    launch_rollout(a, (long long)n * (gh * gw + 1) * ld, L, n, gh, gw, ld, first_layer, map, rec, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_rank_cells(const float* map, int32_t n, int32_t cells, int32_t* rank, void* stream) {
    const char* fn = "fav_op_rank_cells";
    route_clear();
    if (!map || !rank) return op_rejected(fn, "null pointer");
    if (n < 1) return op_rejected(fn, "n must be at least 1");
    if (cells < 1 || cells > CV_MAX_CELLS) return op_rejected(fn, fmt("cells=%d outside [1, %d]", cells, CV_MAX_CELLS).c_str());
    if (((uintptr_t)map | (uintptr_t)rank) & 3) return op_rejected(fn, "map_dev and rank_dev must be 4-byte aligned");
    launch_rank_cells(map, n, cells, rank, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_occlude(const void* frames, void* out, int32_t n, int32_t H, int32_t W, int32_t layout, const int32_t* rank,
                          int32_t mh, int32_t mw, int32_t mode, int32_t S, int32_t s0, int32_t s1, const uint32_t* fill, void* stream) {
    const char* fn = "fav_op_occlude";
    route_clear();
    if (!frames || !out || !rank || !fill) return op_rejected(fn, "null pointer");
    if (n < 1) return op_rejected(fn, "n must be at least 1");
    std::string why = curve_frame_error(H, W, layout);
    if (why.empty()) why = curve_steps_error(S);
    if (why.empty()) why = curve_map_error(mh, mw);
    if (why.empty()) why = curve_mode_error(mode);
    if (why.empty() && (s0 < 0 || s0 >= s1 || s1 > S + 1)) why = fmt("steps [%d, %d) outside 0 <= s0 < s1 <= S + 1 = %d", s0, s1, S + 1);
    if (why.empty()) why = curve_fill_error(fill, layout);
    if (why.empty())
        why = stream_out_error(frames, out, n, H, W, layout, s1 - s0, "(s1 - s0)",
                               (uintptr_t)rank & 3 ? "rank_dev must be 4-byte aligned" : nullptr);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    launch_occlude(frames, out, rank, n, H, W, layout, mh, mw, mode, S, s0, s1, fill, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_head_class_prob(const float* logits, int32_t T, int32_t n, int32_t C, int32_t ld, float temperature,
                                  const int32_t* classes, float* prob, int32_t* labels, void* stream) {
    const char* fn = "fav_op_head_class_prob";
    route_clear();
    if (!logits || !prob) return op_rejected(fn, "null pointer");
    if (T < 1 || T > 4096 || n < 1 || !(temperature > 0.f)) return op_rejected(fn, "needs 1 <= T <= 4096, n >= 1 and temperature > 0");
    const HeadClassProb cp{classes, prob, labels};
    HeadOut out;
    out.cprob = &cp;
    return op_done(fn, launch_head(nullptr, logits, T, n, C, ld, temperature, 0, 0.f, out, (hipStream_t)stream));
}

fav_status fav_op_curve(const float* prob, const int32_t* labels, const int32_t* classes, int32_t n, int32_t S, int32_t cells,
                        int32_t mode, float* curve, fav_curve_record* rec, void* stream) {
    const char* fn = "fav_op_curve";
    route_clear();
    if (!prob || !labels || !classes || !curve || !rec) return op_rejected(fn, "null pointer");
    if (n < 1) return op_rejected(fn, "n must be at least 1");
    std::string why = curve_steps_error(S);
    if (why.empty() && (cells < 1 || cells > CV_MAX_CELLS)) why = fmt("cells=%d outside [1, %d]", cells, CV_MAX_CELLS);
    if (why.empty()) why = curve_mode_error(mode);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)prob | (uintptr_t)labels | (uintptr_t)classes | (uintptr_t)curve) & 3)
        return op_rejected(fn, "prob_dev, labels_dev, classes_dev and curve_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    launch_curve(prob, labels, classes, n, S, cells, mode, 0, curve, rec, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_rise_mask(const void* frames, void* out, int32_t n, int32_t H, int32_t W, int32_t layout, const fav_rise* desc,
                            int64_t first_index, int32_t m0, int32_t m1, void* stream) {
    const char* fn = "fav_op_rise_mask";
    route_clear();
    if (!frames || !out) return op_rejected(fn, "null pointer");
    if (n < 1) return op_rejected(fn, "n must be at least 1");
    std::string why = rise_desc_error(desc, H, W, layout);
    if (why.empty() && (m0 < 0 || m0 >= m1 || m1 > desc->n_masks))
        why = fmt("masks [%d, %d) outside 0 <= m0 < m1 <= n_masks = %d", m0, m1, desc->n_masks);
    if (why.empty()) why = stream_out_error(frames, out, n, H, W, layout, m1 - m0, "(m1 - m0)", nullptr);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    launch_rise_mask(frames, out, n, H, W, layout, *desc, first_index, m0, m1, (hipStream_t)stream);
    return op_done(nullptr);
}

fav_status fav_op_rise_accumulate(const float* prob, const int32_t* classes, int32_t n, const fav_rise* desc, int64_t first_index,
                                  int32_t H, int32_t W, int32_t mh, int32_t mw, int32_t num_classes, float* map, fav_rise_record* rec,
                                  void* stream) {
    const char* fn = "fav_op_rise_accumulate";
    route_clear();
    if (!prob || !classes || !map || !rec) return op_rejected(fn, "null pointer");
    if (n < 1) return op_rejected(fn, "n must be at least 1");
    std::string why = rise_desc_error(desc, H, W, FAV_LAYOUT_NHWC_F32);       // the fill is not read: no byte range to hold it to
    if (why.empty()) why = rise_map_error(mh, mw, H, W);
    if (why.empty() && num_classes < 0) why = fmt("num_classes=%d is negative", num_classes);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)prob | (uintptr_t)classes | (uintptr_t)map) & 3)
        return op_rejected(fn, "prob_dev, classes_dev and map_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    launch_rise_accumulate(prob, classes, n, *desc, first_index, H, W, mh, mw, num_classes, map, rec, (hipStream_t)stream);
    return op_done(nullptr);
}

}  // extern "C"

// ---- the autoencoder anomaly sensor (fav_ae.hpp): an object of its own beside fav_handle ---------------------------
struct fav_ae {
    fav_ae_config cfg;
    AeGeom g;
    int device = 0;
    char* ws = nullptr;              // two rotating activation buffers of g.buf_bytes
    char* slab = nullptr;            // the weights, at the blob's own (64-byte aligned) offsets
    size_t slab_bytes = 0;
    size_t w_off[2 * AE_MAX_LEVELS] = {}, b_off[2 * AE_MAX_LEVELS] = {};
    bool loaded = false;
    float threshold = INFINITY;
};

namespace {
// the blob's size for a level count: the header, the table, every range 64-byte aligned, in table order
size_t ae_blob_bytes(int levels) {
    size_t at = (AE_BLOB_HEADER + 16 * (size_t)(2 * levels) + AE_BLOB_ALIGN - 1) / AE_BLOB_ALIGN * AE_BLOB_ALIGN;
    for (int k = 0; k < 2 * levels; ++k) {
        const AeLayerShape s = ae_layer_shape(levels, k);
        at += (s.w_elems * 2 + AE_BLOB_ALIGN - 1) / AE_BLOB_ALIGN * AE_BLOB_ALIGN;
        at += (s.b_elems * 4 + AE_BLOB_ALIGN - 1) / AE_BLOB_ALIGN * AE_BLOB_ALIGN;
    }
    return at;
}
fav_status ae_rejected(const char* fn, const std::string& why, fav_status st = FAV_ERR_INVALID_ARG) {
    g_create_error = fmt("%s: %s", fn, why.c_str());
    return st;
}
std::string ae_info_error(const fav_ae_config* cfg, AeGeom* g) {
    const std::string why = ae_config_error(cfg);
    if (!why.empty()) return why;
    *g = ae_geometry(*cfg);
    if (g->ws_bytes > AE_MAX_WORKSPACE)
        return fmt("max_batch=%d frames of %d x %d at %d levels need a workspace of %zu bytes, above %zu", cfg->max_batch, cfg->in_h,
                   cfg->in_w, cfg->levels, g->ws_bytes, AE_MAX_WORKSPACE);
    return std::string();
}
}  // namespace

extern "C" {

fav_status fav_check_ae_config(const fav_ae_config* cfg, char* err, size_t err_cap) {
    return check_reply(ae_config_error(cfg), err, err_cap);
}

fav_status fav_ae_info(const fav_ae_config* cfg, int32_t h[4], int32_t w[4], int32_t* gh, int32_t* gw, size_t* workspace_bytes,
                       char* err, size_t err_cap) {
    AeGeom g;
    const std::string why = ae_info_error(cfg, &g);
    if (why.empty()) {
        for (int l = 0; l < 4; ++l) { if (h) h[l] = g.h[l]; if (w) w[l] = g.w[l]; }
        if (gh) *gh = g.gh;
        if (gw) *gw = g.gw;
        if (workspace_bytes) *workspace_bytes = g.ws_bytes;
    }
    return check_reply(why, err, err_cap);
}

fav_status fav_ae_check_blob(const void* blob, size_t size, char* err, size_t err_cap) {
    const std::string why = ae_blob_error(blob, size, nullptr);
    if (err && err_cap) snprintf(err, err_cap, "%s", why.c_str());
    return why.empty() ? FAV_OK : FAV_ERR_BAD_BLOB;
}

fav_status fav_ae_create(const fav_ae_config* cfg, fav_ae** out) {
    const char* fn = "fav_ae_create";
    if (out) *out = nullptr;
    if (!cfg || !out) return ae_rejected(fn, "null argument");
    AeGeom g;
    const std::string why = ae_info_error(cfg, &g);
    if (!why.empty()) return ae_rejected(fn, why);
    int device = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
        (void)hipGetLastError();
        return ae_rejected(fn, "no usable HIP device; this path has no CPU fallback", FAV_ERR_NO_DEVICE);
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ae_rejected(fn, fmt("device %d is '%s', kernels are built for gfx950 only", device, prop.gcnArchName), FAV_ERR_NO_DEVICE);
    fav_ae* ae = new fav_ae();
    ae->cfg = *cfg; ae->g = g; ae->device = device;
    ae->slab_bytes = ae_blob_bytes(cfg->levels);
    if (hipMalloc((void**)&ae->ws, g.ws_bytes) != hipSuccess || hipMalloc((void**)&ae->slab, ae->slab_bytes) != hipSuccess) {
        const std::string e = fmt("cannot allocate %zu + %zu bytes: %s", g.ws_bytes, ae->slab_bytes, hipGetErrorString(hipGetLastError()));
        if (ae->ws) (void)hipFree(ae->ws);
        delete ae;
        return ae_rejected(fn, e, FAV_ERR_HIP);
    }
    *out = ae;
    return FAV_OK;
}

void fav_ae_destroy(fav_ae* ae) {
    if (!ae) return;
    (void)hipSetDevice(ae->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(ae->ws);
    (void)hipFree(ae->slab);
    delete ae;
}

fav_status fav_ae_load_weights(fav_ae* ae, const void* blob, size_t size) {
    const char* fn = "fav_ae_load_weights";
    if (!ae) return ae_rejected(fn, "null object");
    int levels = 0;
    const std::string why = ae_blob_error(blob, size, &levels);
    if (!why.empty()) return ae_rejected(fn, why, FAV_ERR_BAD_BLOB);
    if (levels != ae->cfg.levels)
        return ae_rejected(fn, fmt("the blob has levels=%d, the object was created with levels=%d", levels, ae->cfg.levels), FAV_ERR_BAD_BLOB);
    if (size > ae->slab_bytes) return ae_rejected(fn, fmt("the blob has %zu bytes, its layers need at most %zu", size, ae->slab_bytes), FAV_ERR_BAD_BLOB);
    // the work enqueued on the object may still read the old weights
    if (hipSetDevice(ae->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(ae->slab, blob, size, hipMemcpyHostToDevice) != hipSuccess) {
        ae->loaded = false;
        return ae_rejected(fn, fmt("cannot copy the weights: %s", hipGetErrorString(hipGetLastError())), FAV_ERR_HIP);
    }
    for (int k = 0; k < 2 * levels; ++k) {
        uint64_t off[2];
        memcpy(off, (const uint8_t*)blob + AE_BLOB_HEADER + 16 * (size_t)k, 16);
        ae->w_off[k] = (size_t)off[0]; ae->b_off[k] = (size_t)off[1];
    }
    ae->loaded = true;
    return FAV_OK;
}

fav_status fav_ae_set_threshold(fav_ae* ae, float threshold) {
    if (!ae) return ae_rejected("fav_ae_set_threshold", "null object");
    if (std::isnan(threshold)) return ae_rejected("fav_ae_set_threshold", "threshold is NaN");
    ae->threshold = threshold;
    return FAV_OK;
}

fav_status fav_ae_score(fav_ae* ae, const void* images, int32_t n, int32_t layout, float* err_map, fav_ae_record* rec, uint8_t* recon,
                        void* stream) {
    const char* fn = "fav_ae_score";
    route_clear();
    if (!ae) return ae_rejected(fn, "null object");
    if (!ae->loaded) return ae_rejected(fn, "no weights loaded (fav_ae_load_weights)", FAV_ERR_NO_WEIGHTS);
    if (!images || !err_map || !rec) return ae_rejected(fn, "null pointer");
    if (n < 1 || n > ae->cfg.max_batch) return ae_rejected(fn, fmt("n=%d outside [1, max_batch=%d]", n, ae->cfg.max_batch));
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return ae_rejected(fn, "unknown layout");
    if (layout == FAV_LAYOUT_NHWC_F32 && ((uintptr_t)images & 3)) return ae_rejected(fn, "fp32 frames must be 4-byte aligned");
    if ((uintptr_t)err_map & 3) return ae_rejected(fn, "err_map_dev must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return ae_rejected(fn, "rec_dev must be 8-byte aligned");
    const AeGeom& g = ae->g;
    const int L = g.L, H = ae->cfg.in_h, W = ae->cfg.in_w;
    const std::string dims = ae_decode_dims_error(n, g.h[L], g.w[L], L - 1, H, W, ae->cfg.cell, ae->threshold);
    if (!dims.empty()) return ae_rejected(fn, dims);
    hipStream_t s = (hipStream_t)stream;
    char* buf[2] = {ae->ws, ae->ws + g.buf_bytes};
    int cur = 0;
    static const float kZero3[3] = {0.f, 0.f, 0.f}, kOne3[3] = {1.f, 1.f, 1.f};
    auto refused = [&](const char* e) { return ae_rejected(fn, e); };
    // enc_1: the im2col matrix, then [rows][64] x [64][64]
    if (const char* e = launch_stem(nullptr, images, layout, n, H, W, 3, 3, 2, 1, 64, kZero3, kOne3, buf[cur], s)) return refused(e);
    auto gemm = [&](int k, int frames, int h, int w, int cin, int cout, int ksize, int stride, int pad) -> const char* {
        fav_conv_desc d;
        memset(&d, 0, sizeof d);
        d.x = buf[cur]; d.w = ae->slab + ae->w_off[k]; d.bias = (const float*)(ae->slab + ae->b_off[k]); d.res = nullptr; d.y = buf[cur ^ 1];
        d.n_frames = frames; d.H = h; d.W = w; d.Cin = cin; d.Cout = cout; d.kh = d.kw = ksize; d.stride = stride; d.pad = pad;
        d.relu = 1; d.out_f32 = 0; d.math_mode = FAV_MATH_BF16;
        d.drop.site = -1;
        const char* e = launch_conv(nullptr, d, cout, cout, false, Group{}, s);
        cur ^= 1;
        return e;
    };
    if (const char* e = gemm(0, n, g.h[1], g.w[1], 64, 64, 1, 1, 0)) return refused(e);
    for (int l = 2; l <= L; ++l)
        if (const char* e = gemm(l - 1, n, g.h[l - 1], g.w[l - 1], ae_width(l - 1), ae_width(l), 3, 2, 1)) return refused(e);
    // dec_L .. dec_2: [rows][C_l] x [4 C_{l-1}][C_l], the output read as four times the rows
    int rows_per_frame = g.h[L] * g.w[L];
    for (int l = L; l >= 2; --l) {
        if (const char* e = gemm(2 * L - l, n, rows_per_frame, 1, ae_width(l), 4 * ae_width(l - 1), 1, 1, 0)) return refused(e);
        rows_per_frame *= 4;
    }
    const int k1 = 2 * L - 1;
    launch_ae_decode_compare(buf[cur], n, g.h[L], g.w[L], L - 1, ae->slab + ae->w_off[k1], (const float*)(ae->slab + ae->b_off[k1]), images,
                             layout, H, W, ae->cfg.cell, ae->threshold, nullptr, err_map, rec, recon, s);
    route_clear();
    if (hipGetLastError() != hipSuccess) return ae_rejected(fn, "kernel launch failed", FAV_ERR_HIP);
    return FAV_OK;
}

fav_status fav_op_ae_decode_compare(const void* hidden, int32_t n, int32_t hL, int32_t wL, int32_t m, const void* wg, const float* bias,
                                    const void* frames, int32_t layout, int32_t H, int32_t W, int32_t cell, float threshold,
                                    uint32_t* cell_sse, float* err_map, fav_ae_record* rec, uint8_t* recon, void* stream) {
    const char* fn = "fav_op_ae_decode_compare";
    route_clear();
    if (!hidden || !wg || !bias || !frames || !err_map || !rec) return op_rejected(fn, "null pointer");
    if (layout != FAV_LAYOUT_NHWC_U8 && layout != FAV_LAYOUT_NHWC_F32) return op_rejected(fn, "unknown layout");
    const std::string why = ae_decode_dims_error(n, hL, wL, m, H, W, cell, threshold);
    if (!why.empty()) return op_rejected(fn, why.c_str());
    if (((uintptr_t)hidden | (uintptr_t)wg) & 15) return op_rejected(fn, "hidden_bf16 and wg12_bf16 must be 16-byte aligned");
    if (((uintptr_t)bias | (uintptr_t)err_map | (uintptr_t)cell_sse) & 3) return op_rejected(fn, "bias3, err_map_dev and cell_sse_dev must be 4-byte aligned");
    if (layout == FAV_LAYOUT_NHWC_F32 && ((uintptr_t)frames & 3)) return op_rejected(fn, "fp32 frames must be 4-byte aligned");
    if ((uintptr_t)rec & 7) return op_rejected(fn, "rec_dev must be 8-byte aligned");
    launch_ae_decode_compare(hidden, n, hL, wL, m, wg, bias, frames, layout, H, W, cell, threshold, cell_sse, err_map, rec, recon,
                             (hipStream_t)stream);
    return op_done(nullptr);
}

}  // extern "C"
