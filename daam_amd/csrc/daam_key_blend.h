// daam_key_blend (include/daam_analysis.h) between its kernels and its host entry point (all in daam_key_blend.hip): the
// launch descriptor, the decomposition and the LDS / scratch plan.  The plan is a function of the output's size and n_keys alone --
// the keys' own sizes live on the device --, so the host sizes the launch without reading them back: a key that does not fit the
// staging takes the kernel's gather path instead (same arithmetic, same bits).
#pragma once
#include "daam_key_planes.h"

namespace daam {

constexpr int kBlendThreads = 256;
constexpr int kBlendMaxSets = 8;
constexpr int kBlendChunk = 32;                  // keys of a workgroup: key k belongs to chunk k / kBlendChunk, whatever n_keys is
constexpr int kBlendRows = 4;                    // output rows a lane owns in its column: kBlendMaxSets x kBlendRows accumulators
constexpr size_t kBlendMaxLds = 160 * 1024;

struct BlendLaunch {
    const DaamKeyPlanes* keys;
    const float* weights;                        // [n_sets][n_keys]
    float* out;                                  // set g at out + g * set_stride: [n_rows][out_h][out_w]
    float* part;                                 // scratch behind the flags: [n_chunks][n_sets][n_rows][out_h * out_w]
    int32_t* flags;                              // scratch: [n_sets][n_chunks], 1 = set g has a non-zero weight in the chunk
    int64_t set_stride;
    int32_t n_keys, n_sets, n_rows, out_h, out_w;
    int32_t n_chunks;                            // ceil(n_keys / kBlendChunk); grid y
    int32_t lane_rows;                           // kBlendThreads / out_w: lanes along a column's band
    int32_t band_h;                              // output rows of a workgroup: min(lane_rows * kBlendRows, out_h)
    int32_t n_bands;                             // ceil(out_h / band_h); grid x = n_rows * n_bands
    int32_t stage_cap;                           // floats of the plane's rows, and of the row pass's result, a staged key may use
};

__host__ __device__ inline int blend_chunks(int n_keys) { return (n_keys + kBlendChunk - 1) / kBlendChunk; }
__host__ __device__ inline int blend_band_h(int out_h, int out_w)
{
    const int b = kBlendThreads / out_w * kBlendRows;
    return b < out_h ? b : out_h;
}
// a band of band_h output rows of a key no taller than the output reaches at most band_h + 3 source rows (scale <= 1, four taps)
__host__ __device__ inline int blend_stage_floats(int out_h, int out_w) { return (blend_band_h(out_h, out_w) + 4) * out_w + 8; }
// LDS of a workgroup: the plane's rows | the row pass | the chunk's weights
inline size_t blend_lds_bytes(int out_h, int out_w)
{
    return 4 * (2 * (size_t)blend_stage_floats(out_h, out_w) + kBlendMaxSets * kBlendChunk);
}
// scratch: the flags (padded to 256 bytes), then the partial maps
inline size_t blend_flag_bytes(int n_keys, int n_sets) { return ((size_t)n_sets * blend_chunks(n_keys) * 4 + 255) & ~(size_t)255; }

}  // namespace daam
