// plan_dump - every field of the planner's Plan (csrc/fav_plan.hpp) for a grid of configurations, as text on stdout.
// A host program over the header alone: no library, no device.  It pins the whole plan - not only the schedule text of
// fav_plan_schedule - across a change of the planner, and is what the sanitizers run over:
//
//   g++ -std=c++17 -O1 -o plan_dump tools/plan_dump.cpp                                        (or ROCm's clang++)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o plan_dump_san tools/plan_dump.cpp
//   ./plan_dump | sha256sum        ./plan_dump_san > /dev/null
//
// Per configuration: a "cfg" line; per op the fav_plan_schedule line extended by H W C Ho Wo Co Co2 out_f32 in_elems out_elems;
// per phase "phase <i> op_begin op_end suffix low_res in_elems out_elems out_bytes_per_elem chunk"; per layer its shape; then
// "plan nblocks first_site T_eff cpad has_mc stem_fused" - or "error <status> <text>" where the planner refuses.
//
// Comparing against a library (tools/experiments/plan_dump_parent.diff says how the parent commit's full dump was taken):
//   g++ -std=c++17 -O1 -DPLAN_DUMP_LIBRARY -o plan_dump_lib tools/plan_dump.cpp -ldl
//   ./plan_dump_lib <libfav_hip.so> [flag bits or'ed into fav_plan_schedule's flags]
// prints, for the same grid, what that library's fav_plan_schedule returns.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#ifdef PLAN_DUMP_LIBRARY
#include <dlfcn.h>

#include "../include/fav.h"
static decltype(&fav_plan_schedule) g_plan_schedule;
static int g_flags;
static std::string dump(const fav_config& c, int flags) {
    static char buf[1 << 18];
    const fav_status st = g_plan_schedule(&c, flags | g_flags, buf, sizeof buf);
    return st == FAV_OK ? buf : "error " + std::to_string((int)st) + " " + buf + "\n";
}
#else
#include "../failure_aware_vision_amd/csrc/fav_plan.hpp"
using namespace fav_plan;
static std::string dump(const fav_config& c, int flags) {
    Plan P;
    std::string err, txt;
    char b[512];
    const fav_status st = plan_resnet(c, c.n_members > 1 ? c.n_members : 1, (flags & 1) != 0, &P, &err);
    if (st != FAV_OK) return "error " + std::to_string((int)st) + " " + err + "\n";
    for (size_t pi = 0; pi < P.phases.size(); ++pi)
        for (int i = P.phases[pi].op_begin; i < P.phases[pi].op_end; ++i) {
            const Op& o = P.ops[i];
            snprintf(b, sizeof b, "op %d kind=%d phase=%zu layer=%d lc=%d la=%d in=%d res=%d out=%d out2=%d site=%d relu=%d suffix=%d rese=%d skipy=%d esite=%d"
                     " H=%d W=%d C=%d Ho=%d Wo=%d Co=%d Co2=%d out_f32=%d in_elems=%lld out_elems=%lld\n", i, (int)o.kind, pi, o.layer, o.layer_c, o.layer_a,
                     o.in, o.res, o.out, o.out2, o.site, o.relu, (int)P.phases[pi].suffix, o.res_entry, o.skip_y, P.first_site,
                     o.H, o.W, o.C, o.Ho, o.Wo, o.Co, o.Co2, o.out_f32, o.in_elems, o.out_elems);
            txt += b;
        }
    for (size_t pi = 0; pi < P.phases.size(); ++pi) {
        const Phase& p = P.phases[pi];
        snprintf(b, sizeof b, "phase %zu %d %d %d %d %lld %lld %d %d\n", pi, p.op_begin, p.op_end, (int)p.suffix, (int)p.low_res, p.in_elems, p.out_elems,
                 p.out_bytes_per_elem, p.chunk);
        txt += b;
    }
    for (size_t i = 0; i < P.layers.size(); ++i) {
        const LayerShape& L = P.layers[i];
        snprintf(b, sizeof b, "layer %zu %d %d %d %d %d %d %d %d\n", i, L.cout, L.cin, L.kh, L.kw, L.stride, L.pad, L.cout_pad, L.k);
        txt += b;
    }
    snprintf(b, sizeof b, "plan %d %d %d %d %d %d\n", P.nblocks, P.first_site, P.T_eff, P.cpad, (int)P.has_mc, (int)P.stem_fused);
    return txt + b;
}
#endif

// fav_default_config's values (the planner reads none of the others)
static fav_config base_config(int arch) {
    fav_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.arch = arch;
    c.num_classes = arch == FAV_ARCH_RESNET18_CIFAR ? 10 : 1000;
    c.n_samples = 1;
    c.temperature = 1.f;
    return c;
}

int main(int argc, char** argv) {
#ifdef PLAN_DUMP_LIBRARY
    void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_LOCAL) : nullptr;
    if (!lib || !(g_plan_schedule = (decltype(g_plan_schedule))dlsym(lib, "fav_plan_schedule"))) { fprintf(stderr, "usage: %s <libfav_hip.so> [flags]\n", argv[0]); return 2; }
    g_flags = argc > 2 ? atoi(argv[2]) : 0;
#else
    (void)argc; (void)argv;
#endif
    const int sizes[5][2] = {{8, 8}, {64, 64}, {224, 224}, {240, 320}, {1024, 2048}};
    const int tail_min_rows[3] = {0, -1, 1 << 30}, ens_grouped_max[3] = {0, -1, 16}, chunks[2][2] = {{0, 0}, {7, 3}};
    long long n_cfg = 0;
    for (int arch = 0; arch < 2; ++arch) {
        const int nb = arch ? 16 : 8, d3 = arch ? 3 : 2;      // blocks; blocks of the last stage
        // tests/test_host.py: none, all_blocks, last_layer, layer4+fc, and three odd ones
        const uint32_t l4fc = (1u << nb) | (((1u << (nb - 1)) - 1) & ~((1u << (nb - d3 - 1)) - 1));
        const uint32_t masks[7] = {0, (1u << nb) - 1, 1u << nb, l4fc, 0b101000, 1u << 3, (1u << nb) | 1};
        const int regroups[7] = {-1, 0, 1, 3, 7, 8, nb};
        for (uint32_t mask : masks) for (int T : {3, 30}) for (int regroup : regroups) for (auto& hw : sizes) for (int batch : {1, 32, 256})
        for (int members : {1, 5}) for (int math : {0, 1}) for (int stem : {0, -1}) for (int tmr : tail_min_rows) for (int egm : ens_grouped_max)
        for (auto& ch : chunks) for (int flags : {0, 1}) {
            if (members > 1 && mask != 0) continue;             // fav_create refuses an ensemble with active dropout
            fav_config c = base_config(arch);
            c.site_mask = mask; c.n_samples = T; c.dropout_p = 0.1f; c.regroup_block = regroup; c.in_h = hw[0]; c.in_w = hw[1];
            c.max_batch = batch; c.n_members = members; c.math_mode = math; c.stem_fused = stem; c.tail_min_rows = tmr;
            c.ens_grouped_max = egm; c.chunk_a = ch[0]; c.chunk_b = ch[1];
            printf("cfg arch=%d mask=%u T=%d regroup=%d hw=%dx%d batch=%d members=%d math=%d stem=%d tail_min_rows=%d ens_grouped_max=%d chunks=%d/%d flags=%d\n",
                   arch, mask, T, regroup, hw[0], hw[1], batch, members, math, stem, tmr, egm, ch[0], ch[1], flags);
            fputs(dump(c, flags).c_str(), stdout);
            ++n_cfg;
        }
    }
    fprintf(stderr, "%lld configurations\n", n_cfg);
    return 0;
}
