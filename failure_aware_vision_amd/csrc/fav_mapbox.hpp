// fav_mapbox.hpp - what the two localisation heads share behind their own first scan: cam_kernel (fav_cam.hpp) and
// attn_rollout_kernel (fav_rollout.hpp) each reduce a map of cells to a record of eight dwords whose last two are the count of
// cells at or above a threshold and the box around them.  The threshold rule, the first scan and the other six dwords are each
// head's own contract and stay in its kernel.  Also the budget check of the two user-owned taps that feed the heads.
// Included by fav.hip after fav_route.hpp (fmt), in front of fav_cam.hpp and fav_rollout.hpp.
#pragma once

namespace fav {

using fav_route::fmt;

// ---- host: a tap's buffer against the caller's budget (max_bytes = 0: the tap's default).  what: "maps of max_batch frames take"
inline std::string tap_budget_error(const char* what, size_t bytes, size_t max_bytes, size_t default_budget) {
    const size_t cap = max_bytes ? max_bytes : default_budget;
    if (bytes > cap) return fmt("the %s %zu bytes, above max_bytes=%zu", what, bytes, cap);
    return std::string();
}

// ---- device: one lane's serial scan, in index order, over the cells of a map whose rows are `width` cells: the cells with
//      m[c] >= thr (a NaN cell is not one) are counted and boxed.  Returns the count; *box: x0 | y0 << 8 | x1 << 16 | y1 << 24, or
//      -1 when there is none
__device__ __forceinline__ int map_box_scan(const float* m, int cells, int width, float thr, int* box) {
    int n_above = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int c = 0; c < cells; ++c) {
        if (!(m[c] >= thr)) continue;
        const int y = c / width, x = c - y * width;
        ++n_above;
        x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
    }
    *box = n_above > 0 ? (int)((uint32_t)x0 | ((uint32_t)y0 << 8) | ((uint32_t)x1 << 16) | ((uint32_t)y1 << 24)) : -1;
    return n_above;
}

// the eight dwords of a record (8-byte aligned), as four 8-byte stores
__device__ __forceinline__ void map_record_store(int32_t* rec, int d0, int d1, int d2, int d3, int d4, int d5, int d6, int d7) {
    int2* const out = (int2*)rec;
    out[0] = make_int2(d0, d1);
    out[1] = make_int2(d2, d3);
    out[2] = make_int2(d4, d5);
    out[3] = make_int2(d6, d7);
}

}  // namespace fav
