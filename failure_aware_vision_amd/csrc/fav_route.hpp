// fav_route.hpp — the selector: from the descriptor of a convolution, a bottleneck tail or an attention call to the Route
// fav.hip launches - which kernel instantiation, on what grid, with how much LDS - or to the text of a refusal.  Pure integer
// logic on the host, like the planner it includes: no HIP header, no device, no handle.  fav.hip's launchers only carry a
// Route out; the stand-alone tools/route_dump.cpp prints Routes over a grid of descriptors, and fav_route_* (fav.h) answers
// without a device which kernel a descriptor would take.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "fav_plan.hpp"

namespace fav_route {

using namespace fav_plan;   // FAV_KNOB, conv_out, tail_geometry

enum RouteKind { ROUTE_NONE = 0, ROUTE_CONV_IGEMM, ROUTE_CONV_HALO, ROUTE_PROJ, ROUTE_TAIL, ROUTE_ATTENTION, ROUTE_ENTRY_REDUCE, ROUTE_STEM_POOL };

// One launch: the kernel family and the template arguments that tell its instantiations apart (the key of fav.hip's kernel
// tables and what fav_op_last_route spells), the launch geometry, and the integers the launcher copies into the kernel's
// parameter block.  Or a refusal: then nothing else is filled in.
struct Route {
    int kind = ROUTE_NONE;
    int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool fresh = true;              // fav.hip's report: recorded since the last fav_op_* returned
    const char* refusal = nullptr;
    unsigned grid = 0; int groups = 1;      // blocks; block rows (the members of a grouped launch)
    int block = 0, lds = 0;                 // threads; dynamic LDS bytes
    int patch_bytes = 0;                    // staged-patch 3x3 and tail: the kernel's second argument
    int Ho = 0, Wo = 0, M = 0;              // output frame, rows
    int K = 0, nk = 0, tiles_m = 0, tiles_n = 0, stage_mid = 0;   // ConvParams
    int rs_T = 0, rs_tps = 0;               // TailParams: the res_entry tile order
    TailGeom geom = {};                     // tail and projection: the LDS plan
};

inline Route refuse(const char* why) { Route r; r.refusal = why; return r; }

// printf into a string (fav.hip's messages use it too)
inline std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

inline std::string route_text(const Route& r) {
    const int* a = r.a;
    const char* mode = a[4] ? "f32" : "bf16";
    switch (r.kind) {
    case ROUTE_CONV_IGEMM:    // BM, BN, BK, NS, MODE, EPI, PP, GELU
        return fmt("conv_igemm<%d,%d,%d,%d,%s,epi%d%s%s>", a[0], a[1], a[2], a[3], mode, a[5], a[6] ? ",pp" : "", a[7] ? ",gelu" : "");
    case ROUTE_CONV_HALO:     // CIN, BN, BM, NS, MODE (a[4])
        return fmt("conv3x3_halo<%d,%d,%d,%d,%s>", a[0], a[1], a[2], a[3], mode);
    case ROUTE_PROJ:          // CIN, COUT, NW
        return fmt("proj<%d,%d,nw%d>", a[0], a[1], a[2]);
    case ROUTE_TAIL:          // CMID, NRED, HAS3X3, NW, WC2, RP, RESE
        return fmt("tail<%d,%d,%s,nw%d,wc%d%s%s>", a[0], a[1], a[2] ? "3x3" : "1x1", a[3], a[4] ? 2 : 1, a[5] == 16 ? ",rp16" : "",
                   a[6] ? ",res_entry" : "");
    case ROUTE_ATTENTION:     // MODE, NKT, FULL
        return fmt("attention<%s,%d%s>", a[0] ? "f32" : "bf16", a[1], a[2] ? ",full" : "");
    case ROUTE_ENTRY_REDUCE:  // C, NRED
        return fmt("entry_reduce<%d,%d>", a[0], a[1]);
    case ROUTE_STEM_POOL:     // LAYOUT
        return fmt("stem7_pool<%s>", a[0] ? "f32" : "u8");
    default:
        return std::string();
    }
}

// The one validation of a dropout descriptor (the ranges beside fav_dropout_desc in fav.h), for a launch whose rows are the
// virtual frames [v0, v0 + rows): what is wrong with it, prefixed with the op's name, or nullptr.  A descriptor without a
// site (NULL, site < 0) is not read any further.  The kernels hold v, the sample v / n_img and the fastdiv operand in 32 bits
// (fastdiv is exact below 2^31 only), the draw is 8 bits wide, and scale multiplies every kept value.
inline const char* check_drop(const char* who, const fav_dropout_desc* d, long long rows) {
    if (!d || d->site < 0) return nullptr;
    const char* why = nullptr;
    if (d->threshold > 255u) why = "dropout threshold above 255 (the draw is 8 bits wide: everything would be dropped)";
    else if (!std::isfinite(d->scale) || !(d->scale > 0.f)) why = "dropout scale must be finite and > 0";
    else if (d->n_img < 1) why = "dropout n_img must be >= 1";
    else if (d->v0 < 0 || d->v0 + rows > 0x7fffffffLL) why = "virtual frame index out of range";
    if (!why) return nullptr;
    thread_local std::string msg;
    msg = std::string(who) + ": " + why;
    return msg.c_str();
}

// K-tile depth and ring stages of the 128-row tiles.  Measured on MI355X (profiles/r1d_conv_sweep.txt):
//  * 3x3: MFMA-bound, 64-deep tiles (half the barriers per FLOP), double buffer;
//  * 1x1 with a residual (the expanding convolution of a bottleneck): bound by HBM and by the
//    epilogue; 32-deep tiles with a 3-stage ring (50 KB of LDS -> 3 blocks per CU, which is also
//    what the 143 VGPRs allow);
//  * 1x1 without residual: the same up to K = 256; 64-deep tiles and a double buffer from K = 512.
// FAV_CONV_BK=32|64 forces a value (experiments build).
// Ring depth: three 32-deep stages or two 64-deep ones (the other depths measured no better; their
// instantiations were dropped in round 3).
inline int conv_bk(int kh, int kw, int K, bool has_res) {
    const int forced = (int)FAV_KNOB("FAV_CONV_BK", 0);
    if (forced == 32 || forced == 64) return forced;
    return (kh * kw > 1 || (!has_res && K >= 512) || K >= 1024) ? 64 : 32;   // K >= 1024 with a residual: the ViT MLP's second GEMM
}

// 256 x 256 x 64 tile (8 waves, 128 KB of LDS, one block per CU): twice the FLOPs per
// byte staged from L2, which is what bounds the MFMA-heavy shapes.
// Measured on MI355X it wins on the residual-free 3x3 convolutions and on the 1x1
// convolutions with K >= 512 (+6..25 %), and loses on the shallow 1x1 (K <= 256), whose
// time is the epilogue (nothing overlaps it at one block per CU).  FAV_CONV_BIG: 0 never, 1 always
// when Cout % 256 == 0, unset = the measured rule.
inline bool conv_big(int kh, int kw, long long M, int cout_pad, int K, bool has_res) {
    const int mode = (int)FAV_KNOB("FAV_CONV_BIG", 2);
    const long long min_m = FAV_KNOB("FAV_CONV_BIG_MINM", 8192);
    if (mode == 0 || cout_pad % 256 != 0 || M < min_m) return false;
    if (mode == 1) return true;
    if ((M / 256) * (cout_pad / 256) < 512) return false;   // fewer than two 256x256 tiles per CU: 128-row tiles fill the chip better
    return kh * kw > 1 ? !has_res : K >= 512;
}

// ---- projection shortcut (1x1 / stride s, 256 -> 512, no residual, no ReLU) on the row-owning structure of the tail
//      kernel: every wave gathers the fragments of its 32 output pixels straight from global memory (a strided gather
//      costs nothing there), the 512 output channels stream through as 8 weight chunks, register epilogue.  Measured
//      against the generic kernel on layer 2's shortcut (56x56x256 -> 28x28x512): see profiles/r2e_*.  FAV_PROJ=0 disables.
inline bool proj_enabled() { return FAV_KNOB("FAV_PROJ", 1) != 0; }

// the projection's Route, if the convolution is one it takes (route_conv has checked the descriptor's ranges)
inline bool route_proj(const fav_conv_desc& d, int groups, Route* r) {
    const bool wide = d.Cin == 512 && d.Cout == 1024;       // layer 3's shortcut: 8 waves x 32 pixels, one block per CU
    if (!proj_enabled() || d.kh != 1 || d.kw != 1 || d.pad != 0 || !((d.Cin == 256 && d.Cout == 512) || wide) || d.res || d.drop.site >= 0 ||
        d.out_f32 || d.relu != 0 || d.math_mode != FAV_MATH_BF16 || (d.stride != 1 && d.stride != 2)) return false;
    const int Ho = conv_out(d.H, 1, d.stride, 0), Wo = conv_out(d.W, 1, d.stride, 0);
    const long long M = (long long)d.n_frames * Ho * Wo;
    if (M * groups < (wide ? 512 * 256 : 4096) || M > 0x7fffffffLL || (long long)d.H * d.W * d.Cin * 2 * 4 >= 0x40000000LL) return false;
    r->kind = ROUTE_PROJ;
    r->a[0] = d.Cin; r->a[1] = d.Cout; r->a[2] = wide ? 8 : 4;
    r->Ho = Ho; r->Wo = Wo; r->M = (int)M;
    // [Wc x 2 | bias_b (unused) | bias_c | 256 zero bytes on a 256-byte boundary]
    TailGeom& g = r->geom;
    g.bias_b_off = 2 * 64 * d.Cin * 2; g.bias_ca_off = g.bias_b_off + d.Cin * 5; g.wa_off0 = g.wa_off1 = g.bias_b_off;
    g.zero_off = (g.bias_b_off + (d.Cin + d.Cout) * 5 + 255) & ~255;
    g.lds_bytes = g.zero_off + 256;
    g.nw = r->a[2]; g.rp = 32; g.wc2 = 1;
    r->grid = (unsigned)((M + 32 * g.nw - 1) / (32 * g.nw)); r->groups = groups;
    r->block = 64 * g.nw; r->lds = g.lds_bytes;
    return true;
}

// A convolution whose output rows are cout_pad wide in the weights and ldy apart in memory.  vit: a GEMM of the ViT encoder
// (its own tile rule); groups: the members of a grouped launch - the row thresholds count rows x members.
inline Route route_conv(const fav_conv_desc& d, int cout_pad, int ldy, bool vit, int groups) {
    // conv_out divides by the stride and truncates towards zero: a window larger than the padded frame would come out as
    // Ho = Wo = -1, that is M = n_frames > 0 rows
    if (d.n_frames < 1 || d.H < 1 || d.W < 1) return refuse("conv: n_frames, H and W must be >= 1");
    if (d.kh < 1 || d.kw < 1 || d.stride < 1 || d.pad < 0) return refuse("conv: kh, kw and stride must be >= 1 and pad >= 0");
    if ((long long)d.H + 2ll * d.pad < d.kh || (long long)d.W + 2ll * d.pad < d.kw) return refuse("conv: the window does not fit the padded frame");
    if (d.relu < 0 || d.relu > 2) return refuse("conv: relu must be 0 (none), 1 (ReLU) or 2 (GELU)");
    if (d.out_f32 != 0 && d.out_f32 != 1) return refuse("conv: out_f32 must be 0 or 1");
    if (d.math_mode != FAV_MATH_BF16 && d.math_mode != FAV_MATH_F32_EXACT) return refuse("conv: unknown math_mode");
    if (d.Cin < 64 || d.Cin % 64 != 0) return refuse("conv: Cin must be a multiple of 64 and >= 64");
    if (d.Cout < 1 || cout_pad < d.Cout) return refuse("conv: Cout must be >= 1 and the padded Cout must cover it");   // else tiles_n <= 0: an empty or a wrapped grid
    if (cout_pad % 64 != 0) return refuse("conv: padded Cout must be a multiple of 64");
    // the bf16 epilogues store whole 16-byte groups of channels and range-check rows only: padded columns would land in
    // the next pixel's first channels.  Only the fp32 (logit) output, whose row pitch is the padded width, may be padded.
    if (!d.out_f32 && cout_pad != d.Cout) return refuse("conv: a bf16 output needs Cout to be a multiple of 64 (no column padding)");
    if (d.out_f32 && ldy < cout_pad) return refuse("conv: the fp32 output's row pitch must cover the padded Cout");
    Route r;
    if (cout_pad == d.Cout && ldy == d.Cout && route_proj(d, groups, &r)) return r;
    r.groups = groups;
    r.Ho = conv_out(d.H, d.kh, d.stride, d.pad);
    r.Wo = conv_out(d.W, d.kw, d.stride, d.pad);
    const int HWo = r.Ho * r.Wo;
    const long long M = (long long)d.n_frames * HWo;
    if (M <= 0 || M > 0x7fffffffLL) return refuse("conv: row count out of range");
    r.M = (int)M;
    r.K = d.kh * d.kw * d.Cin;
    if (const char* e = check_drop("conv", &d.drop, d.n_frames)) return refuse(e);
    if (d.out_f32 && d.drop.site >= 0) return refuse("conv: dropout on fp32 output unsupported");
    const int mode = d.math_mode == FAV_MATH_BF16 ? 0 : 1;
    // the ViT encoder's GEMMs (M = 197 rows per frame, K = 768 / 3072): the 256 x 256 tile from 50 of them up (measured, round 4,
    // tools/experiments/r4_vit_tiles.sh: +18 % at 128 frames on two streams, +1.5 % at the 64-frame share; since the GELU epilogue
    // shrank to 14 instructions per element it no longer needs a second block per CU to hide behind); below that 128-row tiles with
    // 32-deep steps at three blocks per CU
    const long long vit_big_tiles = FAV_KNOB("FAV_VIT_BIG_TILES", 50);
    const bool vit_big = vit && cout_pad % 256 == 0 && r.K >= 512 && (M / 256) * (cout_pad / 256) >= vit_big_tiles &&
                         FAV_KNOB("FAV_CONV_BIG", 2) != 0;
    const bool big = vit ? vit_big : conv_big(d.kh, d.kw, M * groups, cout_pad, r.K, d.res != nullptr);   // 256 x 256 x 64 tile, 8 waves, 128 KB of LDS
    const int BN = big ? 256 : ((cout_pad % 128 == 0) ? 128 : 64);
    const int BK = big ? 64 : (vit ? 32 : conv_bk(d.kh, d.kw, r.K, d.res != nullptr));
    const int BM = big ? 256 : 128;   // (256-row tiles with 128 columns lose to two blocks per CU of 128-row tiles on every 3x3 shape)
    // measured: issuing the DMA after the first MFMA group gains ~7 % on the 256x256 3x3 launches and
    // loses 3-5 % on the 128-row tiles and on every 1x1
    r.stage_mid = (big && d.kh * d.kw > 1) ? 1 : 0;
    {   // LDS-DMA offsets are 32-bit from the tile's first frame; out-of-range lanes use 0x80000000
        const double frame_bytes = 2.0 * d.H * d.W * d.Cin;
        const double span = (BM / (double)HWo + 2.0) * frame_bytes + 2.0 * ((double)d.pad * d.W + d.pad) * d.Cin +
                            2.0 * (((double)d.kh * d.W + d.kw) * d.Cin);
        if (span >= 2147483647.0 || 2.0 * BN * (double)r.K >= 2147483647.0) return refuse("conv: frame too large for 32-bit tile offsets");
    }
    r.tiles_m = (r.M + BM - 1) / BM;
    r.tiles_n = cout_pad / BN;
    const long long tiles = (long long)r.tiles_m * r.tiles_n;
    if (tiles > 0x7fffffffLL) return refuse("conv: too many tiles");
    // 3x3 / stride 1 / pad 1 with Cin <= 128 and the whole Cout in one tile: the input patch is staged once
    // per 256 output pixels instead of once per tap (conv3x3_halo_kernel).  FAV_CONV_HALO=0 disables.
    const int halo_mode = (int)FAV_KNOB("FAV_CONV_HALO", 1);
    if (halo_mode && d.kh == 3 && d.kw == 3 && d.stride == 1 && d.pad == 1 && !d.res && d.drop.site < 0 && !d.out_f32 &&
        (d.Cin == 64 || d.Cin == 128) && d.Cout == cout_pad && d.Cout == d.Cin && M * groups >= 2048) {
        // Cin 64: 512-pixel tiles, all 9 K tiles of the weights resident; Cin 128: 256-pixel tiles, weights double-buffered per tap
        // 256-pixel tiles, 8 waves (measured best on both shapes); FAV_HALO_CFG=0 selects 128-pixel tiles with 4 waves and
        // several blocks per CU for experiments
        const int halo_cfg = (int)FAV_KNOB("FAV_HALO_CFG", 1);
        const int HBM = halo_cfg == 0 ? 128 : 256;
        const int wstages = d.Cin == 64 ? (halo_cfg == 0 ? 2 : 3) : (halo_cfg == 0 ? 2 : 4);   // K tiles of weights held in LDS
        const int patch_bytes = (int)((((long long)(HBM + 2 * d.W + 2) * d.Cin * 2) + 1023) / 1024 * 1024);
        const int lds = patch_bytes + wstages * d.Cout * 128 + d.Cout * 5 + 512;   // + 256 zero bytes on a 256-byte boundary
        if (lds <= 160 * 1024) {
            r.kind = ROUTE_CONV_HALO;   // CIN, BN, BM, NS, MODE
            r.a[0] = d.Cin; r.a[1] = d.Cout; r.a[2] = HBM; r.a[3] = (d.Cin == 64 && halo_cfg != 0) ? 3 : 2; r.a[4] = mode;
            r.nk = 9 * d.Cin / 64;
            r.grid = (unsigned)((r.M + HBM - 1) / HBM); r.block = HBM * 2; r.lds = lds; r.patch_bytes = patch_bytes;
            return r;
        }
    }
    r.nk = r.K / BK;
    // FAV_CONV_EPI=0 selects the round-1 epilogue (fp32 staging through LDS) for A/B measurements
    // measured (profiles/r2b_conv_epilogue_ab.txt): the register epilogue wins 2-4 % on the 3x3 and K >= 512 launches
    // (also with a residual on the 256 x 256 tile: layer 4's expand 1.24 vs 1.29 ms) and loses ~3 % on the 128-row
    // tiles with a residual, so those keep the staged one.  FAV_CONV_EPI=0|1 forces.
    const int epi_forced = (int)FAV_KNOB("FAV_CONV_EPI", -1);
    const int epi = epi_forced >= 0 ? epi_forced : ((d.res && !big) ? 0 : 1);
    const int pp = (big && epi && (int)FAV_KNOB("FAV_CONV_PP", 1) && mode == 0) ? 1 : 0;     // the ping-pong K loop: 256 x 256, production mode
    r.kind = ROUTE_CONV_IGEMM;      // BM, BN, BK, NS, MODE, EPI, PP, GELU
    r.a[0] = BM; r.a[1] = BN; r.a[2] = BK; r.a[3] = BK == 32 ? 3 : 2; r.a[4] = mode; r.a[5] = epi ? 1 : 0; r.a[6] = pp; r.a[7] = d.relu == 2;
    r.grid = (unsigned)tiles; r.block = BM * 2;
    return r;
}

// ---- bottleneck tail (conv_b 3x3 -> conv_c 1x1 + residual + dropout -> next block's conv_a 1x1), one launch; its LDS plan
//      is tail_geometry (fav_plan.hpp) ----
inline Route route_tail(const fav_tail_desc& d, int groups) {
    if (d.n_frames < 1 || d.H < 1 || d.W < 1) return refuse("bottleneck tail: n_frames, H and W must be >= 1");
    const bool has3x3 = d.wb != nullptr;
    const int nred = d.wa ? d.Nred : 0;
    Route r;
    TailGeom& g = r.geom;
    if (!tail_geometry(d.Cmid, nred, has3x3, d.W, &g)) return refuse("bottleneck tail: unsupported shape");
    const int HW = d.H * d.W;
    const long long M = (long long)d.n_frames * d.H * d.W;
    if (M <= 0 || M > 0x7fffffffLL) return refuse("bottleneck tail: row count out of range");
    if (const char* e = check_drop("bottleneck tail", &d.drop, d.n_frames)) return refuse(e);
    if (d.res_entry) {
        if (!(d.Cmid == 64 && nred == 64 && has3x3) || d.drop.site < 0 || d.entry_site < 0 || !d.res)
            return refuse("bottleneck tail: res_entry needs Cmid = Nred = 64 with the 3x3 and both dropout sites");
        if ((double)d.drop.n_img * HW * 4.0 * d.Cmid * 2.0 >= 2147483647.0) return refuse("bottleneck tail: cached tensor too large for 32-bit offsets");
    }
    { const int lds_pad = (int)FAV_KNOB("FAV_TAIL_LDS_PAD", 0); if (g.lds_bytes + lds_pad <= 160 * 1024) g.lds_bytes += lds_pad; }   // experiments build: fewer blocks per CU
    const int bm = g.rp * g.nw;
    if (d.res_entry) {
        // whole samples, tiles that do not straddle them: the T tiles over one pixel tile of the cached tensor run back to back
        const bool sample_minor = FAV_KNOB("FAV_ENTRY_RES_ORDER", 1) != 0;
        const long long sample_rows = (long long)d.drop.n_img * HW;
        if (sample_minor && d.drop.v0 % d.drop.n_img == 0 && d.n_frames % d.drop.n_img == 0 && sample_rows % bm == 0) {
            r.rs_T = d.n_frames / d.drop.n_img;
            r.rs_tps = (int)(sample_rows / bm);
        }
    }
    r.kind = ROUTE_TAIL;            // CMID, NRED, HAS3X3, NW, WC2, RP, RESE: the waves, Wc buffers and rows per wave are the LDS plan's
    r.a[0] = d.Cmid; r.a[1] = nred; r.a[2] = has3x3; r.a[3] = g.nw; r.a[4] = g.wc2; r.a[5] = g.rp; r.a[6] = d.res_entry != 0;
    r.Ho = d.H; r.Wo = d.W; r.M = (int)M;
    r.grid = (unsigned)((M + bm - 1) / bm); r.groups = groups;
    r.block = g.nw * 64; r.lds = g.lds_bytes; r.patch_bytes = g.patch_bytes;
    return r;
}

inline Route route_attention(int n, int T, int D, int heads, int math_mode) {
    if (T < 1 || T > 256 || heads * 64 != D || n < 1) return refuse("attention: need 1 <= tokens <= 256 and 64-wide heads");
    const int nkt = (T + 15) / 16, Tp2 = (T + 31) / 32 * 32;
    // as few rounds of query tiles as 8 waves allow, then as few waves as those rounds need (197 tokens: 13 tiles = 2 rounds of 7
    // waves); K and V are all the LDS a block holds (55 KB), so two blocks share a CU
    const int rounds = (nkt + 7) / 8;
    int nw = (nkt + rounds - 1) / rounds;
    const int attn_nw = (int)FAV_KNOB("FAV_ATTN_WAVES", 0);   // experiments build: another block shape
    if (attn_nw >= 1 && attn_nw <= 8) nw = attn_nw;
    Route r;
    r.kind = ROUTE_ATTENTION;       // MODE, NKT, FULL: the kernel compiled for 13 key tiles up to 208 tokens, unmasked at exactly 13 (production mode)
    r.a[0] = math_mode == FAV_MATH_BF16 ? 0 : 1; r.a[1] = nkt <= 13 ? 13 : 16; r.a[2] = r.a[0] == 0 && nkt == 13;
    r.M = T;
    r.grid = (unsigned)(n * heads); r.block = nw * 64; r.lds = nkt * 16 * 128 + Tp2 * 128;
    return r;
}

}  // namespace fav_route
