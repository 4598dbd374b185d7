// Argument block and window table of tap_walk_kernel (daam_tap_walk.hip), shared with the host planner (daam_tap_api.hip).
#pragma once
#include "daam_types.h"

namespace daam {

// One time window of a walk entry: its slice of the layer's running sums, the steps it holds in this launch and whether the
// slice is known to be zero (written, not read).  The step pointers of window w + 1 follow those of window w in TapLaunch::ptrs.
struct WalkWin {
    void* acc;              // [heads_kept, tokens, hw] of this window (ctx acc dtype)
    int32_t n_steps;        // >= 1
    int32_t fresh;
};

// Entry j of the launch (= L.layers[j]: geometry, strides, wg_begin; its n_steps is the total over the entry's windows -- at most
// kMaxStepsPerLaunch -- and its ptr_begin the first window's first step; its acc / fresh are not read) walks wins[win_begin .. + n_win)
struct WalkEntry {
    int32_t win_begin;
    int32_t n_win;
};

struct WalkLaunch {
    TapLaunch L;            // table form only (layers != nullptr)
    const WalkEntry* entries;
    const WalkWin* wins;
};

hipError_t launch_tap_walk(const WalkLaunch&, int in_dtype, int acc_dtype, int fast_exp, hipStream_t, int* grid_out, int* lds_out);
int tap_walk_tile_pixels();

}  // namespace daam
