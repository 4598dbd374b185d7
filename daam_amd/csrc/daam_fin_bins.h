// Window-range reduction of a time-binned context (daam_finalize_bins, include/daam_hip.h): the host side
// (daam_finalize_api.hip) and the kernel (daam_fin_bins.hip) share this table.
#pragma once
#include "daam_finalize.h"

namespace daam {

// One selected key of one group: the planes [0, n_elem) of window bin_begin start at `src`; window w + 1 follows
// `win_stride` ELEMENTS after window w (the windows of a layer are one buffer [n_bins][heads, tokens, side, side]).
// dst[0, n_elem) (f32) = sum over the n_win windows, added in window order.  The task owns the workgroups
// [tile_begin, tile_begin + ceil(n_elem / (256 * V))) of the launch, V = 16 / sizeof(element).
struct BinSumTask {
    const void* src;
    float* dst;
    int64_t win_stride;
    int64_t n_elem;         // rows * side * side: the caller's crop, contiguous from token 0
    int32_t n_win;
    int32_t tile_begin;
    int32_t vec;            // 1: src, dst, win_stride and n_elem allow 16-byte accesses
    int32_t pad;
};

struct BinSumLaunch {
    const BinSumTask* tasks;
    int32_t n_tasks;
    int32_t n_tiles;
};

constexpr int kBinSumThreads = 256;

hipError_t launch_finalize_bin_sum(const BinSumLaunch& L, int dtype, hipStream_t stream);
int bin_sum_elems_per_tile(int dtype);

}  // namespace daam
