// fav_plan.hpp — the planner: from a fav_config to the static schedule fav.hip runs (layer shapes, ops, phases and their pass
// sizes).  Pure integer logic on the host: no HIP header, no device, no handle - fav.hip includes it, and so does the
// stand-alone tools/plan_dump.cpp, which a plain C++ compiler builds (with the sanitizers, if wanted).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/fav.h"

namespace fav_plan {

// Experiment knobs.  A normal build has NONE: every FAV_KNOB is its measured default, a compile-time constant, and the
// library reads no environment variable.  `make EXPERIMENTS=1` (-DFAV_EXPERIMENTS) turns them back into environment variables -
// that build is what tools/*_bench.py, the phase-clock dumps and the A/B records under profiles/ use.  Decided schedule choices
// a caller may want to override are fav_config fields (tail_min_rows, ens_grouped_max, vit_streams, stem_fused), not knobs.
#ifdef FAV_EXPERIMENTS
inline long long fav_knob_read(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }
#define FAV_KNOB(NAME, DFLT) ([] { static const long long v_ = fav_plan::fav_knob_read(NAME, (DFLT)); return v_; }())
#else
#define FAV_KNOB(NAME, DFLT) ((long long)(DFLT))
#endif

struct ArchDef {
    bool bottleneck;
    int depths[4];
    int planes[4];
    bool imagenet_stem;
};
const ArchDef kArch[2] = {
    {false, {2, 2, 2, 2}, {64, 128, 256, 512}, false},
    {true, {3, 4, 6, 3}, {64, 128, 256, 512}, true},
};

struct VitDef { int dim, depth, heads, mlp, patch; };
// arch 2 = ViT-B/16 (BASELINE configs[4]); arch 3 = a two-layer miniature of it for the parity tests
const VitDef kVit[2] = {{768, 12, 12, 3072, 16}, {128, 2, 2, 256, 16}};

struct LayerShape {  // one convolution / fc (ViT, kh == 0: a pair of fp32 vectors of cout values)
    int cout, cin, kh, kw, stride, pad;
    int cout_pad, k;         // device layout: w[cout_pad][k], bias[cout_pad]
};

enum OpKind { OP_STEM_IM2COL, OP_CONV, OP_MAXPOOL, OP_AVGPOOL, OP_ENTRY_DROPOUT, OP_TAIL, OP_ENTRY_REDUCE, OP_STEM_POOL };
enum BufId { B_INPUT = -1, B_PHASE_IN = -2, B_PHASE_OUT = -3, B_NONE = -4, B_A1 = 5 };  // 0..4 rotating

struct Op {
    OpKind kind;
    int layer = -1;          // conv layer index (OP_TAIL: the 3x3, or -1 when the tail starts at the expanding 1x1)
    int layer_c = -1, layer_a = -1;   // OP_TAIL: the expanding 1x1 and the NEXT block's reducing 1x1 (-1: none)
    int in = B_NONE, out = B_NONE, res = B_NONE;
    int out2 = B_NONE;       // OP_TAIL: the next block's conv1 output
    int Co2 = 0;
    int H = 0, W = 0, C = 0;           // input dims per frame
    int Ho = 0, Wo = 0, Co = 0;        // output dims per frame
    int relu = 0, out_f32 = 0;
    int site = -1;                     // dropout site fused into this op
    int res_entry = 0;                 // OP_TAIL: the residual is the cached prefix output under the entry dropout (RESE)
    int skip_y = 0;                    // OP_ENTRY_REDUCE: the dropped copies are not stored (the next tail recomputes them)
    int stage_out = 0;                 // 1 .. 4: `out` is the output of that residual stage's last block (the stage tap's); 0: not
    long long in_elems = 0, out_elems = 0;  // per frame
};

struct Phase {
    int op_begin, op_end;
    bool suffix;             // operates on virtual frames (t, i)
    long long in_elems, out_elems;   // per (virtual) frame
    int out_bytes_per_elem;
    bool low_res;            // belongs to the low-resolution group (chunk_b)
    int chunk;               // (virtual) frames per pass
};
const int kMaxPhases = 4;    // prefix and suffix, each split at most once (at the low-resolution group)

struct Plan {
    std::vector<LayerShape> layers;  // in blob order
    std::vector<Op> ops;             // ResNet archs: the launches of one pass, in order
    std::vector<Phase> phases;
    int nblocks = 0;
    int first_site = -1;             // the dropout site the suffix starts behind (-1: no MC-Dropout)
    int T_eff = 1;                   // samples actually run
    int cpad = 0;                    // row pitch of the logits
    bool has_mc = false, stem_fused = false;   // what will_group asks about the schedule
    int ntok = 0;                    // ViT archs: tokens per frame
};

inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }

// ---- bottleneck tail (conv_b 3x3 -> conv_c 1x1 + residual + dropout -> next block's conv_a 1x1), one launch ----
struct TailGeom { int patch_bytes, rega_bytes, lds_bytes, nw, wc2, rp, bias_b_off, bias_ca_off, wa_off0, wa_off1, zero_off; };
// LDS plan of bottleneck_tail_kernel<CMID, NRED, HAS3X3, NS, NW, WC2> (must match the kernel's own layout)
inline bool tail_geometry(int cmid, int nred, bool has3x3, int W, TailGeom* g) {
    const int cout = 4 * cmid;
    // default plan behind the weight buffers: bias_b | bias_c | bias_a | 256 zero bytes on a 256-byte boundary
    auto finish = [&](int bias_b_off, int wa_off0, int wa_bytes) {
        g->bias_b_off = bias_b_off; g->bias_ca_off = bias_b_off + cmid * 5;
        g->wa_off0 = wa_off0; g->wa_off1 = wa_off0 + wa_bytes;
        g->zero_off = (bias_b_off + (cmid + cout + nred) * 5 + 255) & ~255;
        g->lds_bytes = g->zero_off + 256;
    };
    if (cmid == 512) {      // layer 4: the expanding 1x1 alone
        if (has3x3 || nred != 0) return false;
        // 8 waves x 32 pixels, Wc double-buffered (2 x 64 KB), one block per CU: 1.14 ms against 1.24 ms for 4 waves with a
        // single Wc buffer at two blocks per CU and 1.27 ms for the generic kernel (profiles/r2j_tail_l4.txt)
        g->patch_bytes = 0; g->rega_bytes = 0; g->nw = 8; g->rp = 32; g->wc2 = 1;
        finish(2 * 65536, 2 * 65536, 0);
        return true;
    }
    if (cmid == 256) {      // layer 3: the expanding 1x1 alone, or with the next block's reduce (then 8 waves x 16 rows)
        if ((has3x3 && nred != 0) || !(nred == 0 || nred == 256)) return false;
    } else if ((cmid != 64 && cmid != 128) || !(nred == 0 || nred == cmid || nred == 128)) return false;
    if (cmid == 256 && has3x3) {
        // conv_b as the generic 256 x 256 x 64 loop (two 64 KB stages); T2, then the Wc buffers, reuse those 128 KB
        g->patch_bytes = 0; g->rega_bytes = 128 * 1024; g->nw = 8; g->rp = 32; g->wc2 = 1;
        finish(g->rega_bytes, g->rega_bytes, 0);
        return true;
    }
    const int rp = (cmid == 256 && nred == 256) ? 16 : 32;
    const int rowb = cmid * 2, ns = cmid == 64 ? 3 : 2;
    const int wc_bytes = 64 * rowb, wa_bytes = nred * 128;
    auto plan = [&](int nw) {
        const int bm = rp * nw;
        const int patch = has3x3 ? (int)((((long long)(bm + 2 * W + 2) * rowb) + 1023) / 1024 * 1024) : 0;
        // region A: patch | T2 tile | Y chunk; without conv_b the T2 fragments come straight from global memory
        int rega = has3x3 ? std::max(std::max(patch, bm * 128), bm * rowb) : (nred > 0 ? bm * 128 : 0);
        rega = (rega + 1023) / 1024 * 1024;
        const int ring = has3x3 ? ns * cmid * 128 : 0;
        const int budget = nw == 4 ? 80 * 1024 : 160 * 1024;
        g->patch_bytes = patch; g->rega_bytes = rega; g->nw = nw; g->rp = rp;
        // Wc double-buffered when two blocks still fit a CU (4-wave blocks) / the block fits at all (8-wave blocks)
        g->wc2 = 1;
        int regb = std::max(ring, 2 * wc_bytes + 2 * wa_bytes);
        finish(rega + regb, rega + 2 * wc_bytes, wa_bytes);
        if (g->lds_bytes > budget) {
            g->wc2 = 0;
            regb = std::max(ring, wc_bytes + 2 * wa_bytes);
            finish(rega + regb, rega + wc_bytes, wa_bytes);
        }
        return g->lds_bytes <= budget;
    };
    // Waves per block (pixels per block = 32 * waves).  64 mid channels: 4 waves (128 pixels, two blocks per CU; an 8-wave / 256-pixel
    // variant measured the same, profiles/r2a_tail_bench.txt); 128 mid channels: 8 waves (256 pixels, one block per CU; 4-wave blocks
    // at two per CU - 81 920 B each with a compact LDS plan - are bit-identical and within 1 %: profiles/r4d_l2_tail_two_blocks_per_cu.txt);
    // 256 (conv_c alone): 4 waves, two blocks per CU.
    return plan((cmid == 128 || (cmid == 256 && nred == 256)) ? 8 : 4);
}

// The fused tails at all (FAV_FUSE=0: the layer-by-layer schedule, as in the validation math mode)
inline bool tail_enabled() { return FAV_KNOB("FAV_FUSE", 1) != 0; }
// 256 mid channels (layer 3): the expanding 1x1 + residual + dropout on the row-owning structure.  FAV_TAIL_WIDE=0 disables.
inline bool tail_wide() { return FAV_KNOB("FAV_TAIL_WIDE", 1) != 0; }
// 256 mid channels: conv_b (generic loop) + conv_c in one launch.  FAV_TAIL_WIDE3X3=0 keeps the 3x3 as its own launch.
inline bool tail_wide3x3() { return FAV_KNOB("FAV_TAIL_WIDE3X3", 1) != 0; }
// 512 mid channels (layer 4): the expanding 1x1 + residual + dropout on the row-owning structure.  FAV_TAIL_L4=0 disables.
inline bool tail_l4() { return FAV_KNOB("FAV_TAIL_L4", 1) != 0; }

// Entry dropout + the 1x1 reduce behind it (entry_reduce_kernel): 256 -> 64 channels, the first dropout site of the
// all_blocks policy.  FAV_ENTRY_FUSE=0 keeps the two launches.
inline bool entry_reduce_enabled() { return FAV_KNOB("FAV_ENTRY_FUSE", 1) != 0; }
inline bool entry_reduce_supported(int C, int nred, long long n_img, long long HW) {
    return C == 256 && nred == 64 && n_img * HW * C * 2 < 0x70000000LL;     // 32-bit byte offsets into the cached tensor
}
// The block behind the entry reduce: its tail can take its residual - the dropped copy of the cached prefix output - from the
// cached tensor itself and apply the entry mask in its epilogue; the T copies are then neither written (12 GB per step at the
// headline shape) nor read back.  FAV_ENTRY_RES=0 keeps them.
inline bool entry_res_enabled() { return FAV_KNOB("FAV_ENTRY_RES", 1) != 0; }

// A deep ensemble runs every op as ONE launch over its members (run_grouped) when: there is no MC-Dropout suffix, the production
// math mode, the one-launch stem (every op is then one the grouped kernels cover), fav_config.ens_grouped_max >= 0 - and the call
// has at most ens_grouped_max frames.  The one predicate: classify_on_stream asks it with the call's frames; the planner, which
// plans the size-dependent tail kernels of layers 3-4 for max_batch frames, asks whether a call of max_batch frames will be grouped.
inline bool will_group(const fav_config& c, int n_members, const Plan& P, int frames) {
    if (n_members <= 1 || P.has_mc || c.math_mode != FAV_MATH_BF16 || !P.stem_fused || c.ens_grouped_max < 0) return false;
    return c.ens_grouped_max == 0 || frames <= c.ens_grouped_max;
}

inline int add_layer(Plan& P, int cout, int cin, int kh, int kw, int stride, int pad) {
    P.layers.push_back({cout, cin, kh, kw, stride, pad, (cout + 63) / 64 * 64, kh * kw * cin});
    return (int)P.layers.size() - 1;
}

// ------------------------------------------------------------------ ResNet archs
// One walk over the network, front to back; every op is final when it is emitted (its buffers, its dropout site), and a phase
// is final when it is closed.  What the walk needs to know ahead - the first dropout site, where the low-resolution group
// starts, how many members a planned launch covers - plan_resnet works out before the first op.
struct ResNetWalk {
    const fav_config& c;
    const ArchDef& A;
    Plan& P;
    const bool fusable;      // fused tails and the entry reduce: production math mode only, and not in the layer-by-layer schedule
    const int groups;        // members a planned launch of max_batch frames covers (an ensemble without MC-Dropout, see will_group)
    const int regroup;       // the block in front of which the low-resolution group starts (nblocks: the pool; -1: nowhere)
    const bool entry_alone;  // the entry op takes no reduce (see plan_resnet)
    int H, W, C = 64;        // the current activation ...
    int cur = 0;             // ... and the rotating buffer that holds it
    int pre_t1 = -1;         // rotating buffer already holding the coming block's conv1 output
    int entry_reduce = -1;   // the OP_ENTRY_REDUCE just emitted, while the block behind it is being walked
    int ph_begin = 0, ph_src = B_NONE;          // the open phase: its first op, the rotating buffer its input was left in
    bool ph_suffix = false, ph_low = false;

    static int other(std::initializer_list<int> used) {     // the first rotating buffer not in use
        for (int i = 0; i < 5; ++i)
            if (std::find(used.begin(), used.end(), i) == used.end()) return i;
        return -1;
    }
    // dropout site s (block s's output; nblocks: the pooled features) if it is drawn by the op that computes it: the sites
    // behind the first one (the first is the entry op's)
    int site_at(int s) const { return P.has_mc && s > P.first_site && (c.site_mask >> s & 1) ? s : -1; }

    // the one place that fills an op's dimensions and element counts
    Op& emit(OpKind kind, int layer, int in, int out, int Hi, int Wi, int Ci, int Ho, int Wo, int Co) {
        Op o; o.kind = kind; o.layer = layer; o.in = in; o.out = out;
        o.H = Hi; o.W = Wi; o.C = Ci; o.Ho = Ho; o.Wo = Wo; o.Co = Co;
        o.in_elems = (long long)Hi * Wi * Ci; o.out_elems = (long long)Ho * Wo * Co;
        P.ops.push_back(o);
        return P.ops.back();
    }
    Op& conv(int layer, int in, int out, int res, int relu, int Hi, int Wi) {
        const LayerShape& L = P.layers[layer];
        Op& o = emit(OP_CONV, layer, in, out, Hi, Wi, L.cin, conv_out(Hi, L.kh, L.stride, L.pad), conv_out(Wi, L.kw, L.stride, L.pad), L.cout);
        o.res = res; o.relu = relu;
        return o;
    }

    // The open phase ends in front of the next op: its last op writes the phase output, and the ops that read the rotating
    // buffer its input was left in - until somebody overwrites that buffer - read the phase input instead.
    void close_phase() {
        const int b = ph_begin, e = (int)P.ops.size();
        if (b >= e) return;
        for (int k = b; k < e && ph_src != B_NONE; ++k) {
            Op& o = P.ops[k];
            if (o.in == ph_src) o.in = B_PHASE_IN;
            if (o.res == ph_src) o.res = B_PHASE_IN;
            if (o.out == ph_src || o.out2 == ph_src) break;
        }
        Phase p; p.op_begin = b; p.op_end = e; p.suffix = ph_suffix; p.low_res = ph_low;
        p.in_elems = P.ops[b].in_elems;
        p.out_elems = P.ops[e - 1].out_elems;
        p.out_bytes_per_elem = P.ops[e - 1].out_f32 ? 4 : 2;
        long long pe = 1;       // the largest tensor an op of the phase writes
        for (int k = b; k < e; ++k) pe = std::max(pe, P.ops[k].out == B_A1 ? P.ops[k].out_elems / 2 : P.ops[k].out_elems);
        // Pass size: measured on MI355X, fewer and larger launches beat
        // keeping producer->consumer tensors inside the 256 MiB Infinity Cache at every
        // size tried (launch ramp/tail cost more than the HBM round trip), so by default a
        // phase runs all its frames in one pass, bounded by a 16 GiB-per-tensor arena
        // budget (5 rotating tensors; 288 GB of HBM makes that a non-issue).
        // (Running the last two phases as a two-stream pipeline - the low-resolution phase of chunk c beside the high-resolution
        // phase of chunk c+1 - measured 119.0-121.2 ms per step against 118.5 ms without; the code is gone, its
        // record is tools/experiments/phase_pipeline_two_streams.diff.)
        const int want = ph_low ? c.chunk_b : c.chunk_a;
        const long long chunk = want > 0 ? want : std::max<long long>(1, (16ll << 30) / (pe * 2));
        const long long dom = (long long)c.max_batch * (ph_suffix ? P.T_eff : 1);
        p.chunk = (int)std::max<long long>(1, std::min(chunk, dom));
        P.ops[e - 1].out = B_PHASE_OUT;
        P.phases.push_back(p);
        ph_begin = e;
    }
    void low_res_from_here() { close_phase(); ph_low = true; ph_src = cur; }

    // stem: one launch in the production math mode (normalise, 7x7/2, ReLU, max pool); else im2col (normalise fused) + dense
    // GEMM over the padded patch matrix (+ max pool)
    void stem() {
        const int sk = A.imagenet_stem ? 7 : 3, ss = A.imagenet_stem ? 2 : 1, sp = A.imagenet_stem ? 3 : 1;
        const int li = add_layer(P, 64, 3, sk, sk, ss, sp);
        const int K = P.layers[li].k = (sk * sk * 3 + 63) / 64 * 64;  // device K is the padded patch length
        const int Ho = conv_out(H, sk, ss, sp), Wo = conv_out(W, sk, ss, sp);
        const int Hp = conv_out(Ho, 3, 2, 1), Wp = conv_out(Wo, 3, 2, 1);
        if (P.stem_fused) {
            emit(OP_STEM_POOL, li, B_INPUT, cur, H, W, 3, Hp, Wp, 64).relu = 1;
        } else {
            emit(OP_STEM_IM2COL, li, B_INPUT, B_A1, H, W, 3, Ho, Wo, K);
            emit(OP_CONV, li, B_A1, cur, Ho, Wo, K, Ho, Wo, 64).relu = 1;
            if (A.imagenet_stem) { emit(OP_MAXPOOL, -1, cur, other({cur}), Ho, Wo, 64, Hp, Wp, 64); cur = P.ops.back().out; }
        }
        H = A.imagenet_stem ? Hp : Ho; W = A.imagenet_stem ? Wp : Wo;
    }

    // residual block b: `pl` planes, 3x3 stride `stride`; next_pl: the planes of the block behind it (0: none); stage_end:
    // the residual stage (1 .. 4) this block is the last of, else 0
    void block(int b, int pl, int stride, int next_pl, int stage_end) {
        if (b == regroup) low_res_from_here();
        const int Hn = conv_out(H, 3, stride, 1), Wn = conv_out(W, 3, stride, 1), exp = A.bottleneck ? 4 : 1;
        const bool ds = stride != 1 || C != pl * exp;       // projection shortcut
        if (A.bottleneck) bottleneck(b, pl, stride, ds, next_pl, Hn, Wn);
        else basic(pl, stride, ds, Hn, Wn);
        P.ops.back().site = site_at(b);
        P.ops.back().stage_out = stage_end;
        entry_reduce = -1;
        H = Hn; W = Wn; C = pl * exp;
    }

    void basic(int pl, int stride, bool ds, int Hn, int Wn) {
        const int xin = cur, t1 = other({xin}), t2 = other({xin, t1});
        const int l1 = add_layer(P, pl, C, 3, 3, stride, 1), l2 = add_layer(P, pl, pl, 3, 3, 1, 1);
        conv(l1, xin, t1, B_NONE, 1, H, W);
        int idn = xin;
        if (ds) { idn = t2; conv(add_layer(P, pl, C, 1, 1, stride, 0), xin, idn, B_NONE, 0, H, W); }
        cur = conv(l2, t1, other({xin, t1, idn}), idn, 1, Hn, Wn).out;
    }

    void bottleneck(int b, int pl, int stride, bool ds, int next_pl, int Hn, int Wn) {
        const int inpl = C, xin = cur;
        const int t1 = pre_t1 >= 0 ? pre_t1 : other({xin}), t2 = other({xin, t1});
        const int l1 = add_layer(P, pl, inpl, 1, 1, 1, 0), l2 = add_layer(P, pl, pl, 3, 3, stride, 1), l3 = add_layer(P, pl * 4, pl, 1, 1, 1, 0);
        const int ld = ds ? add_layer(P, pl * 4, inpl, 1, 1, stride, 0) : -1;
        if (pre_t1 < 0) conv(l1, xin, t1, B_NONE, 1, H, W);   // else: written by the previous block's fused tail / the entry reduce
        pre_t1 = -1;
        // Fused tail (bottleneck_tail_kernel): conv2 (when 3x3/1) + conv3 (+ the NEXT block's conv1 unless a
        // phase boundary or the end of the network lies between the two blocks).  Production math mode only.
        const bool boundary_after = b + 1 == P.nblocks || b == P.first_site || b + 1 == regroup;
        int nred = boundary_after ? 0 : next_pl;
        // the 256-pixel / 8-wave kernels of layers 3-4 run one block per CU: they pay only when the planned launch
        // (max_batch frames, x T samples behind the first dropout site) brings two blocks per CU
        // (an ensemble without MC-Dropout runs every op as one launch over its members, see run_grouped)
        const long long plan_rows = (long long)c.max_batch * ((P.has_mc && b > P.first_site) ? c.n_samples : 1) * Hn * Wn * groups;
        const bool big_launch = c.tail_min_rows < 0 || plan_rows >= (c.tail_min_rows > 0 ? (long long)c.tail_min_rows : 512ll * 256);
        const bool tail_3x3 = stride == 1 && (pl <= 128 || (pl == 256 && tail_wide3x3() && big_launch));
        if (pl > 128) nred = 0;   // wide blocks: the expanding 1x1 alone (with the next block's reduce in the launch it measured 3.01 ms against 1.77 + 0.95: only fav_op_bottleneck_tail still reaches that kernel)
        bool fuse = fusable && (pl == 64 || pl == 128 || (pl == 256 && tail_wide()) || (pl == 512 && tail_l4() && big_launch));
        TailGeom tg;
        if (fuse && !tail_geometry(pl, nred, tail_3x3, Wn, &tg)) {
            nred = 0;
            fuse = tail_geometry(pl, 0, tail_3x3, Wn, &tg);
        }
        int t2v = t1;
        if (!(fuse && tail_3x3)) {                          // the 3x3 as its own launch
            conv(l2, t1, t2, B_NONE, 1, H, W);
            t2v = t2;
        }
        int idn = xin;
        // blob order is conv1, conv2, conv3, downsample; launch order: downsample before conv3
        if (ds) { idn = other({xin, t1, t2}); conv(ld, xin, idn, B_NONE, 0, H, W); }
        if (!fuse) {
            cur = conv(l3, t2, ds ? other({xin, t1, t2, idn}) : t1, idn, 1, Hn, Wn).out;   // t1 is dead after conv2
            return;
        }
        const int yout = other({xin, t1, t2v, idn});    // t2 is free when the 3x3 is fused, xin when it is not the residual
        Op& o = emit(OP_TAIL, tail_3x3 ? l2 : -1, t2v, yout, Hn, Wn, pl, Hn, Wn, pl * 4);
        o.layer_c = l3; o.res = idn; o.relu = 1; o.Co2 = nred;
        if (nred > 0) { o.layer_a = (int)P.layers.size(); o.out2 = pre_t1 = other({t2v, idn, yout}); }   // the next add_layer() is the next block's conv1
        // Behind the entry reduce the residual - this block's input - is the dropped copy of the cached prefix output.
        // Nobody else reads the copies: a block reads its input, what it wrote itself and what the tail in front of it
        // left, so with this tail taking them from the cached tensor the entry reduce need not store them.
        if (entry_reduce >= 0 && entry_res_enabled() && !ds && tail_3x3 && pl == 64 && nred == 64 && site_at(b) >= 0 &&
            (double)c.max_batch * H * W * inpl * 2.0 < 2147483647.0) { o.res_entry = 1; P.ops[entry_reduce].skip_y = 1; }
        cur = yout;
    }

    // The suffix starts here, with the entry dropout of the cached prefix output - written where the prefix's last op left
    // that output, which is where the ops behind read it.  The 1x1 reduce that follows (a bottleneck's conv1, next_pl planes)
    // joins the dropout launch.
    void entry(int next_pl) {
        close_phase();
        ph_suffix = true; ph_src = B_NONE;
        Op o; o.kind = OP_ENTRY_DROPOUT; o.in = B_PHASE_IN; o.out = cur; o.site = P.first_site;
        o.in_elems = o.out_elems = (long long)H * W * C;
        if (fusable && entry_reduce_enabled() && !entry_alone && next_pl > 0 && entry_reduce_supported(C, next_pl, c.max_batch, (long long)H * W)) {
            o.kind = OP_ENTRY_REDUCE; o.layer_a = (int)P.layers.size(); o.out2 = pre_t1 = other({cur}); o.Co2 = next_pl;
            o.H = H; o.W = W; o.C = C; o.relu = 1;
            entry_reduce = (int)P.ops.size();
        }
        P.ops.push_back(o);
    }

    void pool_fc() {
        if (regroup == P.nblocks) low_res_from_here();
        emit(OP_AVGPOOL, -1, cur, other({cur}), H, W, C, 1, 1, C).site = site_at(P.nblocks);
        cur = P.ops.back().out; H = W = 1;
        if (P.first_site == P.nblocks) entry(0);
        const int lfc = add_layer(P, c.num_classes, C, 1, 1, 1, 0);
        P.cpad = P.layers[lfc].cout_pad;
        Op& o = conv(lfc, cur, other({cur}), B_NONE, 0, 1, 1);
        o.out_f32 = 1; o.out_elems = P.cpad;
        close_phase();
    }
};

// The schedule of a ResNet arch (0, 1).  no_fuse: the layer-by-layer schedule (the fused one's reference, fav_plan_schedule).
inline fav_status plan_resnet(const fav_config& c, int n_members, bool no_fuse, Plan* out, std::string* err) {
    const ArchDef& A = kArch[c.arch];
    Plan P;
    const int sk = A.imagenet_stem ? 7 : 3, ss = A.imagenet_stem ? 2 : 1, sp = A.imagenet_stem ? 3 : 1;
    const int Hs = conv_out(c.in_h, sk, ss, sp), Ws = conv_out(c.in_w, sk, ss, sp);
    if (Hs < 1 || Ws < 1) { *err = "input too small"; return FAV_ERR_INVALID_ARG; }
    P.nblocks = A.depths[0] + A.depths[1] + A.depths[2] + A.depths[3];
    const uint32_t valid_mask = (P.nblocks + 1 >= 32) ? 0xFFFFFFFFu : ((1u << (P.nblocks + 1)) - 1);
    if (c.site_mask & ~valid_mask) { *err = "site_mask has bits beyond the pooled-feature site"; return FAV_ERR_INVALID_ARG; }
    // dropout sites: the ops up to the first one are the prefix, run once per frame; the suffix runs T times
    P.has_mc = c.site_mask != 0 && std::lround((double)c.dropout_p * 256.0) > 0;
    P.T_eff = P.has_mc ? c.n_samples : 1;
    for (int s = 0; P.has_mc && P.first_site < 0; ++s)
        if (c.site_mask >> s & 1) P.first_site = s;
    // production math mode: the whole ImageNet stem is one launch
    P.stem_fused = A.imagenet_stem && c.math_mode == FAV_MATH_BF16 && c.stem_fused >= 0 && !no_fuse &&
                   conv_out(Hs, 3, 2, 1) >= 1 && conv_out(Ws, 3, 2, 1) >= 1;
    // The low-resolution group (chunk_b) starts in front of this block; the fused tails must not straddle it.  Directly behind
    // the entry op it starts nowhere - a phase is split only with a real op on each side, so the suffix stays one
    // high-resolution phase - and the entry op then takes no reduce either.
    int regroup = std::min(c.regroup_block < 0 ? A.depths[0] + A.depths[1] : c.regroup_block, P.nblocks);
    const bool entry_alone = P.has_mc && regroup == P.first_site + 1;
    if (entry_alone) regroup = -1;
    const bool fusable = tail_enabled() && !no_fuse && c.math_mode == FAV_MATH_BF16;
    ResNetWalk w{c, A, P, fusable, will_group(c, n_members, P, c.max_batch) ? n_members : 1, regroup, entry_alone, c.in_h, c.in_w};
    w.stem();
    for (int st = 0, b = 0; st < 4; ++st)
        for (int bi = 0; bi < A.depths[st]; ++bi, ++b) {
            const int next_pl = bi + 1 < A.depths[st] ? A.planes[st] : (st < 3 ? A.planes[st + 1] : 0);
            w.block(b, A.planes[st], (bi == 0 && st > 0) ? 2 : 1, next_pl, bi + 1 == A.depths[st] ? st + 1 : 0);
            if (b == P.first_site) w.entry(A.bottleneck ? next_pl : 0);
        }
    w.pool_fc();
    if (P.phases.size() > (size_t)kMaxPhases) { *err = "schedule has more phases than a lane holds"; return FAV_ERR_UNSUPPORTED; }
    *out = std::move(P);
    return FAV_OK;
}

// ------------------------------------------------------------------ ViT archs
// Layers in blob order (kh == 0: a pair of fp32 vectors), fixed buffers, no phases (single deterministic pass).
inline fav_status plan_vit(const fav_config& c, Plan* out, std::string* err) {
    const VitDef& V = kVit[c.arch - 2];
    if (c.in_h % V.patch || c.in_w % V.patch) { *err = "ViT input must be a multiple of the patch size"; return FAV_ERR_INVALID_ARG; }
    Plan P;
    P.ntok = (c.in_h / V.patch) * (c.in_w / V.patch) + 1;
    if (P.ntok > 256) { *err = "ViT path supports at most 256 tokens"; return FAV_ERR_UNSUPPORTED; }
    if (c.site_mask != 0 && c.dropout_p > 0.f) { *err = "the ViT path has no dropout sites"; return FAV_ERR_UNSUPPORTED; }
    if (c.n_members > 1) { *err = "the ViT path has no ensemble mode"; return FAV_ERR_UNSUPPORTED; }
    auto lin = [&](int cout, int cin, int kh, int kw, int stride) { add_layer(P, cout, cin, kh, kw, stride, 0); };
    auto vec = [&](int len) { P.layers.push_back({len, 0, 0, 0, 0, 0, len, 0}); };
    lin(V.dim, 3, V.patch, V.patch, V.patch);
    vec(P.ntok * V.dim);
    for (int i = 0; i < V.depth; ++i) {
        vec(V.dim); lin(3 * V.dim, V.dim, 1, 1, 1); lin(V.dim, V.dim, 1, 1, 1);
        vec(V.dim); lin(V.mlp, V.dim, 1, 1, 1); lin(V.dim, V.mlp, 1, 1, 1);
    }
    vec(V.dim);
    lin(c.num_classes, V.dim, 1, 1, 1);
    P.cpad = P.layers.back().cout_pad;
    *out = std::move(P);
    return FAV_OK;
}

}  // namespace fav_plan
