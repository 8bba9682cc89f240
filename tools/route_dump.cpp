// route_dump - what the selector (csrc/fav_route.hpp) answers for a grid of descriptors, as text on stdout.  A host program
// over the header alone: no library, no device.  It pins every Route - the kernel AND its launch geometry - across a change
// of the selector, and is what the sanitizers run over:
//
//   g++ -std=c++17 -O1 -o route_dump tools/route_dump.cpp                                      (or ROCm's clang++)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o route_dump_san tools/route_dump.cpp
//   ./route_dump | sha256sum        ./route_dump_san > /dev/null
//
// Per descriptor one line: a tag that spells the descriptor, then
//   "<route name> grid=<x>x<members> block=<threads> lds=<bytes> patch=<bytes> nk=<n> tiles=<m>x<n> stage_mid=<0|1> rs=<T>/<tiles per sample>"
// or "error <text>" where the selector refuses.
//
// Comparing against a library (tools/experiments/route_dump_parent.diff says how the parent commit's dump was taken):
//   g++ -std=c++17 -O1 -DROUTE_DUMP_LIBRARY -o route_dump_lib tools/route_dump.cpp -ldl
//   ./route_dump_lib <libfav_hip.so>
// prints, for the same grid, what that library's fav_route_dump_* entry points (the patch adds them) return.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#ifdef ROUTE_DUMP_LIBRARY
#include <dlfcn.h>

#include "../include/fav.h"
static fav_status (*g_conv)(const fav_conv_desc*, int32_t, int32_t, int32_t, int32_t, char*, size_t);
static fav_status (*g_tail)(const fav_tail_desc*, int32_t, char*, size_t);
static fav_status (*g_attn)(int32_t, int32_t, int32_t, int32_t, int32_t, char*, size_t);
static char g_buf[512];
static std::string line_conv(const fav_conv_desc& d, int cout_pad, int ldy, int vit, int groups) { g_conv(&d, cout_pad, ldy, vit, groups, g_buf, sizeof g_buf); return g_buf; }
static std::string line_tail(const fav_tail_desc& d, int groups) { g_tail(&d, groups, g_buf, sizeof g_buf); return g_buf; }
static std::string line_attention(int n, int T, int D, int heads, int mode) { g_attn(n, T, D, heads, mode, g_buf, sizeof g_buf); return g_buf; }
#else
#include "../failure_aware_vision_amd/csrc/fav_route.hpp"
using namespace fav_route;
static std::string line(const Route& r) {
    if (r.refusal) return std::string("error ") + r.refusal;
    char b[256];
    snprintf(b, sizeof b, " grid=%ux%d block=%d lds=%d patch=%d nk=%d tiles=%dx%d stage_mid=%d rs=%d/%d", r.grid, r.groups, r.block, r.lds, r.patch_bytes,
             r.nk, r.tiles_m, r.tiles_n, r.stage_mid, r.rs_T, r.rs_tps);
    return route_text(r) + b;
}
static std::string line_conv(const fav_conv_desc& d, int cout_pad, int ldy, int vit, int groups) { return line(route_conv(d, cout_pad, ldy, vit != 0, groups)); }
static std::string line_tail(const fav_tail_desc& d, int groups) { return line(route_tail(d, groups)); }
static std::string line_attention(int n, int T, int D, int heads, int mode) { return line(route_attention(n, T, D, heads, mode)); }
#endif

static char g_mem[64];      // what the descriptors' pointers point at; the selector tests them for NULL and never reads them
static long long g_lines;

static fav_dropout_desc no_drop() {
    fav_dropout_desc dd;
    memset(&dd, 0, sizeof dd);
    dd.site = -1; dd.scale = 1.f; dd.n_img = 1;
    return dd;
}

struct ConvCase { int n, H, W, cin, cout, kh, kw, stride, pad, res, relu, out_f32, mode; };
static void conv(const ConvCase& c, int vit, int groups, const fav_dropout_desc& dd, int cout_pad = -1, int ldy = -1) {
    fav_conv_desc d;
    memset(&d, 0, sizeof d);
    d.x = d.w = d.y = g_mem; d.bias = (const float*)g_mem; d.res = c.res ? g_mem : nullptr;
    d.n_frames = c.n; d.H = c.H; d.W = c.W; d.Cin = c.cin; d.Cout = c.cout; d.kh = c.kh; d.kw = c.kw; d.stride = c.stride; d.pad = c.pad;
    d.relu = c.relu; d.out_f32 = c.out_f32; d.math_mode = c.mode; d.drop = dd;
    if (cout_pad < 0) cout_pad = c.cout;
    if (ldy < 0) ldy = c.cout;
    printf("conv n=%d %dx%d %d->%d(%d,%d) k%dx%d s%d p%d res%d relu%d f32out%d mode%d site%d thr%u scale%g n_img%d v0=%lld vit%d g%d: %s\n", c.n, c.H, c.W, c.cin,
           c.cout, cout_pad, ldy, c.kh, c.kw, c.stride, c.pad, c.res, c.relu, c.out_f32, c.mode, dd.site, dd.threshold, (double)dd.scale, dd.n_img,
           (long long)dd.v0, vit, groups, line_conv(d, cout_pad, ldy, vit, groups).c_str());
    ++g_lines;
}

struct TailCase { int n, H, W, cmid, nred, wb, wa, res_entry, entry_site, res; };
static void tail(const TailCase& c, int groups, const fav_dropout_desc& dd) {
    fav_tail_desc d;
    memset(&d, 0, sizeof d);
    d.x = d.wc = d.y = g_mem; d.bias_c = (const float*)g_mem; d.res = c.res ? g_mem : nullptr;
    if (c.wb) { d.wb = g_mem; d.bias_b = (const float*)g_mem; }
    if (c.wa) { d.wa = g_mem; d.bias_a = (const float*)g_mem; d.t1n = g_mem; }
    d.n_frames = c.n; d.H = c.H; d.W = c.W; d.Cmid = c.cmid; d.Nred = c.nred; d.drop = dd; d.res_entry = c.res_entry; d.entry_site = c.entry_site;
    printf("tail n=%d %dx%d cmid%d nred%d wb%d wa%d rese%d esite%d res%d site%d thr%u n_img%d v0=%lld g%d: %s\n", c.n, c.H, c.W, c.cmid, c.nred, c.wb, c.wa,
           c.res_entry, c.entry_site, c.res, dd.site, dd.threshold, dd.n_img, (long long)dd.v0, groups, line_tail(d, groups).c_str());
    ++g_lines;
}

int main(int argc, char** argv) {
#ifdef ROUTE_DUMP_LIBRARY
    void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_LOCAL) : nullptr;
    if (lib) {
        g_conv = (decltype(g_conv))dlsym(lib, "fav_route_dump_conv2d");
        g_tail = (decltype(g_tail))dlsym(lib, "fav_route_dump_bottleneck_tail");
        g_attn = (decltype(g_attn))dlsym(lib, "fav_route_dump_attention");
    }
    if (!g_conv || !g_tail || !g_attn) { fprintf(stderr, "usage: %s <libfav_hip.so with fav_route_dump_*>\n", argv[0]); return 2; }
#else
    (void)argc; (void)argv;
#endif
    const fav_dropout_desc none = no_drop();
    fav_dropout_desc site3 = none;
    site3.site = 3; site3.threshold = 26; site3.scale = 1.1f; site3.v0 = 3; site3.n_img = 4;

    // ---- convolutions.  Frames: one row; 143 rows (the conv tables' generic shape, both strides); both sides of 2048 rows
    // (staged-patch 3x3; 32 x 64 against 64 x 32: the LDS fit at 128 channels), of 4096 (projection), of 8192 rows and of 512 big
    // tiles at Cout 2048 (16384 rows) and 512 (65536 rows); and the same thresholds at rows x members with 2 and 5 members
    const int frames[][3] = {{1, 1, 1}, {1, 11, 13}, {1, 21, 25}, {1, 23, 89}, {1, 89, 23}, {1, 32, 64}, {1, 64, 32}, {1, 31, 33}, {1, 32, 32},
                             {1, 409, 1}, {1, 10, 41}, {1, 63, 65}, {1, 64, 64}, {1, 125, 129}, {1, 127, 127}, {1, 9, 91}, {1, 20, 41}, {1, 90, 91},
                             {1, 64, 128}, {1, 36, 91}, {1, 29, 113}, {1, 127, 129}, {1, 128, 128}, {1, 125, 132}, {240, 16, 17}, {241, 16, 17},
                             {672, 28, 28}, {700, 14, 14}, {2, 15, 15}, {2, 9, 11}};
    const int windows[][4] = {{1, 1, 1, 0}, {1, 1, 2, 0}, {3, 3, 1, 1}, {3, 3, 2, 1}, {7, 7, 2, 3}, {1, 3, 1, 0}, {3, 1, 1, 1}};
    for (int cin : {64, 128, 256, 512, 1024}) for (int cout : {64, 128, 192, 256, 320, 512, 1024, 2048}) for (auto& w : windows)
    for (int res : {0, 1}) for (int relu : {0, 1, 2}) for (int mode : {0, 1}) for (int f32 : {0, 1}) for (auto& f : frames)
    for (int vit : {0, 1}) for (int groups : {1, 2, 5})
        conv({f[0], f[1], f[2], cin, cout, w[0], w[1], w[2], w[3], res, relu, f32, mode}, vit, groups, none);
    // the ViT encoder's GEMMs: 197 rows per frame; K below 512, 768 and 3072; the 49 / 50 big-tile boundary itself at one
    // column tile (12 799 against 12 800 rows) and crossed at 3, 9 and 12 column tiles; the padded fp32 logits
    const int vit_frames[][2] = {{1, 1}, {1, 197}, {6, 197}, {7, 197}, {8, 197}, {22, 197}, {23, 197}, {64, 197}, {128, 197}, {1, 12799}, {1, 12800}};
    for (int k : {256, 512, 768, 3072}) for (int cout : {256, 768, 1024, 2304, 3072}) for (auto& f : vit_frames) for (int res : {0, 1})
    for (int relu : {0, 2}) for (int mode : {0, 1}) for (int vit : {0, 1}) for (int groups : {1, 2, 5}) {
        conv({f[0], f[1], 1, k, cout, 1, 1, 1, 0, res, relu, 0, mode}, vit, groups, none);
        if (cout == 1024) conv({f[0], f[1], 1, k, 1000, 1, 1, 1, 0, res, relu, 1, mode}, vit, groups, none, 1024, 1024);
    }
    // the 256 x 256 tile's 8192-row minimum alone: at 32 column tiles the tile count is met long before
    for (auto& f : {frames[11], frames[12]}) for (int res : {0, 1}) for (int mode : {0, 1}) for (int groups : {1, 2, 5})
        conv({f[0], f[1], f[2], 512, 8192, 1, 1, 1, 0, res, 1, 0, mode}, 0, groups, none);
    // a dropout site in the epilogue (no staged-patch 3x3, no projection), and what the selector refuses, in its order
    for (int cin : {64, 256}) for (int cout : {64, 512}) for (auto& w : windows) for (int f32 : {0, 1}) for (auto& f : frames)
        conv({f[0], f[1], f[2], cin, cout, w[0], w[1], w[2], w[3], 1, 1, f32, 0}, 0, 1, site3);
    const ConvCase ok = {1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 1, 0, 0};
    auto refused = [&](ConvCase c, const fav_dropout_desc& dd, int cout_pad = -1, int ldy = -1) { conv(c, 0, 1, dd, cout_pad, ldy); };
    { ConvCase c = ok; c.n = 0; refused(c, none); c = ok; c.H = -8; refused(c, none); c = ok; c.W = 0; refused(c, none); }
    { ConvCase c = ok; c.kh = 0; refused(c, none); c = ok; c.stride = 0; refused(c, none); c = ok; c.pad = -1; refused(c, none); }
    { ConvCase c = ok; c.H = 1; c.W = 1; c.pad = 0; refused(c, none); c = ok; c.H = 1; c.kh = 7; c.kw = 1; c.pad = 2; refused(c, none); }
    { ConvCase c = ok; c.relu = 3; refused(c, none); c = ok; c.out_f32 = 2; refused(c, none); c = ok; c.mode = 2; refused(c, none); }
    { ConvCase c = ok; c.cin = 96; refused(c, none); c.cin = 0; refused(c, none); c = ok; c.cout = 0; refused(c, none); c.cout = -64; refused(c, none); }
    { ConvCase c = ok; c.cout = 100; refused(c, none, 64, 64); refused(c, none, 100, 100); refused(c, none, 128, 128); c.out_f32 = 1; refused(c, none, 128, 100); }
    { ConvCase c = ok; c.n = 1000; c.H = c.W = 2048; refused(c, none); c = ok; c.H = c.W = 8192; refused(c, none); }
    { ConvCase c = ok; c.n = 32767; c.H = c.W = 256; c.cout = 16384; c.kh = c.kw = 1; c.pad = 0; refused(c, none); }
    { fav_dropout_desc dd = site3; dd.threshold = 256; refused(ok, dd); dd = site3; dd.scale = 0.f; refused(ok, dd); dd = site3; dd.n_img = 0; refused(ok, dd); }
    { fav_dropout_desc dd = site3; dd.v0 = -1; refused(ok, dd); dd.v0 = 0x7fffffffLL; refused(ok, dd); ConvCase c = ok; c.out_f32 = 1; refused(c, site3); }

    // ---- bottleneck tails: every (Cmid, Nred, 3x3) arm and the unsupported ones; W across the ranges where the patch leaves room
    // for two Wc buffers, for one, and for none (64/64: W 116..147 one; 64/128: 52..83; 128/128: 56..87)
    const int widths[] = {1, 7, 14, 28, 51, 52, 55, 56, 83, 84, 87, 88, 115, 116, 147, 148, 200, 300, 600, 5000};
    for (int cmid : {64, 96, 128, 256, 512}) for (int nred : {0, 64, 128, 256}) for (int wb : {0, 1}) for (int wa : {0, 1}) for (int W : widths)
    for (int H : {1, 7, 56}) for (int n : {1, 3, 37}) for (int groups : {1, 2, 5}) for (int drop : {0, 1})
        tail({n, H, W, cmid, nred, wb, wa, 0, 0, 1}, groups, drop ? site3 : none);
    // res_entry (tests/test_gpu_tail.py's cases, and chunks of whole samples of whole tiles - the sample-minor order - against not)
    const int rese[][5] = {{56, 56, 3, 0, 9}, {20, 12, 4, 2, 9}, {7, 9, 5, 13, 37}, {60, 80, 2, 1, 3}, {16, 16, 2, 4, 6}, {8, 16, 3, 0, 6}, {56, 56, 4, 0, 12},
                           {3, 120, 2, 1, 5}, {3, 120, 2, 2, 6}, {16, 16, 2, 3, 6}, {16, 16, 2, 4, 5}, {16, 8, 4, 4, 8}, {16, 8, 1, 0, 1}, {16, 9, 1, 0, 7}};
    for (auto& c : rese) for (int groups : {1, 2}) {
        fav_dropout_desc dd = site3;
        dd.n_img = c[2]; dd.v0 = c[3];
        tail({c[4], c[0], c[1], 64, 64, 1, 1, 1, 2, 1}, groups, dd);
    }
    tail({6, 16, 16, 64, 64, 1, 1, 1, 2, 1}, 1, none);                  // no dropout site of its own
    tail({6, 16, 16, 64, 64, 1, 1, 1, -1, 1}, 1, site3);                // no entry site
    tail({6, 16, 16, 64, 64, 1, 1, 1, 2, 0}, 1, site3);                 // no cached tensor
    tail({6, 16, 16, 128, 128, 1, 1, 1, 2, 1}, 1, site3); tail({6, 16, 16, 64, 64, 0, 1, 1, 2, 1}, 1, site3); tail({6, 16, 16, 64, 128, 1, 1, 1, 2, 1}, 1, site3);
    { fav_dropout_desc dd = site3; dd.n_img = 20000; tail({6, 56, 56, 64, 64, 1, 1, 1, 2, 1}, 1, dd); dd = site3; dd.threshold = 300; tail({6, 16, 16, 64, 64, 1, 1, 1, 2, 1}, 1, dd); }
    tail({0, 8, 8, 64, 0, 1, 0, 0, 0, 1}, 1, none); tail({2, -56, 8, 64, 0, 1, 0, 0, 0, 1}, 1, none); tail({1000, 2048, 2048, 64, 0, 1, 0, 0, 0, 1}, 1, none);

    // ---- attention: every token count and two beyond, both math modes; heads that are not 64 wide, no frames
    for (int T = 0; T <= 258; ++T) for (int mode : {0, 1}) for (int n : {1, 3}) for (int heads : {2, 12}) {
        printf("attention n=%d T=%d heads%d mode%d: %s\n", n, T, heads, mode, line_attention(n, T, heads * 64, heads, mode).c_str());
        ++g_lines;
    }
    for (int T : {1, 197}) {
        printf("attention n=1 T=%d D=704 heads12: %s\n", T, line_attention(1, T, 704, 12, 0).c_str());
        printf("attention n=0 T=%d D=768 heads12: %s\n", T, line_attention(0, T, 768, 12, 0).c_str());
        g_lines += 2;
    }
    fprintf(stderr, "%lld descriptors\n", g_lines);
    return 0;
}
