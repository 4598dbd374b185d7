// daam_key_scores (include/daam_analysis.h) between its kernel and its host entry point (both in daam_key_scores.hip):
// the launch descriptor and the LDS plan.  The plan is a function of the output's size alone -- the keys' own sizes live on the
// device --, so the host can size the launch without reading them back: a key that does not fit the staging takes the kernel's
// gather path instead (same arithmetic, same bits).
#pragma once
#include "daam_key_planes.h"

namespace daam {

constexpr int kKsThreads = 256;
constexpr int kKsMaxBatch = 4;                   // token rows whose clamped tiles a workgroup holds while the footprints stream by
constexpr int kKsMaskGroup = 4;                  // footprints a lane carries at once: kKsMaskGroup x kKsMaxBatch accumulators
constexpr int kKsMaxMasks = 32;
constexpr size_t kKsMaxLds = 160 * 1024;
constexpr size_t kKsTwoPerCu = 80 * 1024;        // at most this much per workgroup: two of them share a CU

struct KsLaunch {
    const DaamKeyPlanes* keys;
    const float* footprint;                      // [n_masks][out_h][out_w], or NULL (n_masks == 0: the total mass)
    float* scores;                               // [n_keys][max(n_masks, 1)][n_rows]
    int32_t n_keys, n_rows, out_h, out_w, n_masks;
    int32_t batch;                               // tiles in LDS, 1 .. kKsMaxBatch
    int32_t chunk_rows;                          // token rows of a workgroup (a multiple of batch, or every row)
    int32_t n_chunks;                            // workgroups per key; grid = n_keys * n_chunks
    int32_t tmp_cap;                             // floats of the row pass's result a staged key may use
};

// floats of one tile (16-byte aligned), of the row-pass buffer (an x2 key's h * out_w is exactly half the tile), of one tap table
__host__ __device__ inline int ks_tile_floats(int out_h, int out_w) { return (out_h * out_w + 3) & ~3; }
__host__ __device__ inline int ks_tmp_floats(int out_h, int out_w) { return ((out_h * out_w + 1) / 2 + 3) & ~3; }
__host__ __device__ inline int ks_tab_entries(int out_h, int out_w) { return (out_h + out_w) * 4; }
// LDS of a workgroup: [batch] tiles | tmp | tap weights | tap indices | the waves' partial sums
inline size_t ks_lds_bytes(int out_h, int out_w, int batch)
{
    return 4 * ((size_t)batch * ks_tile_floats(out_h, out_w) + ks_tmp_floats(out_h, out_w) + 2 * (size_t)ks_tab_entries(out_h, out_w) +
                kKsMaskGroup * kKsMaxBatch * (kKsThreads / 64));
}

}  // namespace daam
