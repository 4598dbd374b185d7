// finalize_rect_kernel (daam_finalize_rect.hip): the launch descriptors of the finalize for planes and outputs of unequal sides.
#pragma once
#include "daam_finalize.h"

namespace daam {

// One selected (layer, head) key: planes [tokens, h, w], position p = pixel (p / w, p % w).
struct FinRectKey {
    const void* base;       // plane of token 0
    int16_t h, w;
    int32_t tab;            // index of the (h, w) table pair (-1: h == out_h && w == out_w, copy + clamp)
};

// Table pair `tab`, [out_w + out_h][4] entries: the row table bicubic_table(w, out_w) (entries [0, out_w)), then the column
// table bicubic_table(h, out_h).
struct FinRectLaunch {
    const FinRectKey* keys;
    const int16_t* tab_idx;
    const float* tab_w;
    float* out;             // [tokens, out_h, out_w]
    int32_t n_keys;
    int32_t n_chunks;
    int32_t tokens;         // token rows of the call (grid x)
    int32_t out_h, out_w;
    int32_t plane_cap;      // floats of the LDS plane region (largest h * w of a key with a table, rounded up to 4)
    float inv_n;
};

struct FinRectGroupLaunch {
    FinRectLaunch L;        // shared fields; keys / n_keys / tokens / inv_n / out are per group (fin_rect_group_view)
    FinGroup g[kFinMaxGroups];
};

__host__ __device__ inline FinRectLaunch fin_rect_group_view(const FinRectGroupLaunch& G, int g)
{
    FinRectLaunch L = G.L;
    L.keys += G.g[g].key_begin;
    L.n_keys = G.g[g].n_keys;
    L.tokens = G.g[g].rows;
    L.inv_n = G.g[g].inv_n;
    L.out += G.g[g].out_off;
    return L;
}

// LDS floats of a launch: the output tile, the plane and the row-pass result [h][out_w] (tmp_cap = largest h * out_w).
inline size_t fin_rect_lds_bytes(int out_h, int out_w, int plane_cap, int tmp_cap)
{
    return sizeof(float) * ((((size_t)out_h * out_w + 3) & ~size_t(3)) + (size_t)plane_cap + (size_t)tmp_cap);
}
constexpr size_t kFinRectMaxLds = 160 * 1024;   // LDS a gfx950 workgroup can have

// G == NULL: finalize_rect_kernel on L; otherwise L is G->L and finalize_rect_grouped_kernel runs on *G with grid z = n_groups
hipError_t launch_finalize_rect(const FinRectLaunch& L, const FinRectGroupLaunch* G, int n_groups, int tmp_cap, int dtype,
                                hipStream_t stream, int* grid_out, int* lds_out);

}  // namespace daam
