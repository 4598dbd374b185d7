/* daam_analysis.h -- C ABI of libdaam_analysis.so: head analysis on the MI355X (gfx950).
 *
 * The reference gives DiffusionHeatMapHooker.compute_global_heat_map its head_idx= / layer_idx= arguments
 * (daam/trace.py:103-126) so that one can ask which heads and layers carry a word: per selected (factor, layer, head)
 * key the running sum is resized to the map's size (bicubic), clamped at 0 and -- for a score -- weighed inside an image
 * region, which is what WordHeatMap.expand_as(absolute=True) (daam/heatmap.py:77-93) followed by a masked sum gives.
 * The clamp sits between the bicubic and the sum over keys, so per-key scores cannot be taken from the global map;
 * this library computes them from ONE read of the running sums, without writing a map per key:
 *
 *   scores[k][m][t] = sum_p footprint[m][p] * max(bicubic(plane_k,t -> out_h x out_w)[p], 0)        t in [0, n_rows)
 *
 * Conventions: those of daam_hip.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t
 * passed as void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_analysis_last_error() gives the
 * message of the last failure on the calling thread.  The library holds no context and no state between calls, and works
 * on the HIP device that is current.  It is separate from libdaam_hip.so and needs nothing from it but this header's
 * include of daam_hip.h (the DAAM_E_* and dtype codes).
 */
#ifndef DAAM_ANALYSIS_H
#define DAAM_ANALYSIS_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_ANALYSIS_ABI_VERSION 1

typedef struct DaamKeyPlanes {     /* one (layer, head) key; DEVICE array */
    const void* base;              /* planes [>= n_rows][h][w], contiguous, of window 0 of the range; any element alignment */
    int64_t     win_stride;        /* ELEMENTS from window i to window i + 1 (ignored when n_win == 1) */
    int32_t     h, w;              /* 1 <= h, w <= 128, any ratio to the output (x4, x2, x1, x0.5, non-square) */
    int32_t     n_win;             /* >= 1: the planes of n_win windows are added in f32, in window order, BEFORE the bicubic */
    int32_t     pad;
} DaamKeyPlanes;

/* Per-key region scores.  `keys` [n_keys] on the device; `dtype` (DAAM_F16 | DAAM_F32 | DAAM_BF16) is the planes' element type;
 * `footprint` [n_masks][out_h][out_w] fp32 is what daam_region_scores leaves behind (the masks pulled back onto the map's grid;
 * negative lobes are normal); `scores` [n_keys][max(n_masks, 1)][n_rows] fp32 is overwritten in full.  n_masks == 0 with
 * footprint == NULL: one column, the total clamped mass (footprint == 1; nothing is read for it, and the result equals an
 * all-ones footprint bit for bit).
 *
 * The bicubic is F.interpolate(mode='bicubic', align_corners=False): rows first, then columns, border-clamped taps, Keys'
 * weights with A = -0.75 in f32 -- the order of the non-square finalize.  A key whose plane has the output's size is clamp
 * only.  f32 arithmetic throughout: any finite planes, err <= 2^-19 * rowmax per resized element, and for a score
 *     |got - exact| <= e_t * sum_p |f_m[p]| + c * 2^-24 * sum_p |f_m[p] * K[p]|
 * with e_t = (2^-19 + 2 (n_win - 1) 2^-24) * rowmax_t (rowmax_t: the largest |window sum| of the row's plane, every partial
 * sum included; each of the n_win - 1 f32 additions per element is off by <= 2^-24 of a partial sum, and the 16 tap weights
 * of an output element sum to <= 1.375^2 < 2 in absolute value) and c = 2 + ceil(out_h * out_w / 256) + 8: the product's rounding, the
 * clamp's input, and the longest chain of additions of the fixed tree below.
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): 1 <= n_keys <= 2^20, 0 <= n_masks <= 32,
 * 1 <= out_h, out_w <= 128, 1 <= n_rows, dtype one of the three, keys / scores not NULL, footprint NULL exactly when
 * n_masks == 0.  DAAM_E_UNSUPPORTED when the workgroup's dynamic LDS would exceed 160 KB.  A key whose h, w or n_win is
 * outside its range is not read: its scores are NaN.
 *
 * Deterministic: no floating-point atomics; one workgroup owns each (key, token row) result; a lane adds its elements
 * p = lane, lane + 256, ... in ascending order, a butterfly joins the 64 lanes of a wave, the four waves are added as
 * (w0 + w1) + (w2 + w3).  scores[k] is bit-identical from run to run and does not depend on the other keys of the call, on
 * n_rows, on n_masks or on where a plane starts in memory.  Rows at or past n_rows are never read. */
DAAM_API int daam_key_scores(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, int out_h, int out_w,
                             const float* footprint, int n_masks, float* scores, void* stream);
DAAM_API int daam_analysis_abi_version(void);          /* DAAM_ANALYSIS_ABI_VERSION */
DAAM_API const char* daam_analysis_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
