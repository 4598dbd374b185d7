/* daam_blend.h -- C ABI of libdaam_blend.so: heat maps from a chosen, weighted set of (layer, head) keys on the MI355X (gfx950).
 *
 * daam_key_scores and daam_token_gram (daam_analysis.h) say WHICH keys matter; daam_key_blend makes the map of a chosen set of them.
 * It is the finalize's arithmetic (compute_global_heat_map, reference daam/trace.py:116-126) with a weight per key in front of the
 * sum over keys, for up to 8 weight sets from ONE read of the running sums:
 *
 *   out[g][t][p] = sum_k  w[g][k] * max(bicubic(plane_k,t -> out_h x out_w)[p], 0)        t in [0, n_rows),  g in [0, n_sets)
 *
 * The clamp sits between the bicubic and the sum over keys, so this cannot be derived from the global map or from per-key scores.
 * With w = 1 / n_keys it is the global heat map of the same keys.
 *
 * Conventions: those of daam_analysis.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t passed
 * as void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_blend_last_error() gives the message of the last
 * failure on the calling thread.  The library holds no context and no state between calls and works on the HIP device that is
 * current.  It is separate from libdaam_hip.so and libdaam_analysis.so and needs nothing from them but their headers (DaamKeyPlanes,
 * the DAAM_E_* and dtype codes).
 */
#ifndef DAAM_BLEND_H
#define DAAM_BLEND_H

#include "daam_analysis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_BLEND_ABI_VERSION 1

/* Weighted sum of clamped, resized key planes.  `keys` [n_keys] on the device, the descriptors of daam_key_scores; `dtype`
 * (DAAM_F16 | DAAM_F32 | DAAM_BF16) is the planes' element type; `weights` [n_sets][n_keys] fp32 on the device; `out` holds set g
 * at out + g * set_stride (ELEMENTS) as [n_rows][out_h][out_w] fp32 and is overwritten in full; `scratch` holds the chunks'
 * partial maps and is the caller's between calls.
 *
 * Bicubic.  F.interpolate(mode='bicubic', align_corners=False): rows first, then columns, border-clamped taps, Keys' weights with
 * A = -0.75, all in f32, every product and sum rounded on its own -- the order of daam_key_scores.  A key's plane may be x4, x2,
 * x1 or x0.5 of the output (any ratio, in fact), and need not be square; a key of the output's size is clamp only.  Any finite
 * planes: err <= 2^-19 * rowmax per resized element (the class of daam_hip.h).
 *
 * Windows.  n_win > 1 adds the windows' planes in f32, in window order, BEFORE the bicubic: the arithmetic of daam_key_scores.
 *
 * Zero weights.  A zero weight is NO CONTRIBUTION, not 0 x value: a key that set g weighs 0 cannot reach out[g], even when its
 * planes hold NaN or Inf.  A key weighed 0 by every set of the call is not read at all, so ten keys out of 1100 cost about ten
 * keys.  (-0.0 is a zero weight.)  Under a non-zero weight the clamp keeps a NaN, as torch's does: a set that weighs a key of
 * NaN planes is NaN where that key's map is.
 *
 * Descriptor range.  A key whose h, w (1..128) or n_win (>= 1) is out of range is never read: every set that gives it a non-zero
 * weight is NaN in all its rows, the other sets are untouched.
 *
 * Weights.  Any finite f32, negative ones included; nothing is normalised on the device.
 *
 * Error, per output element, with e_k,t = (2^-19 + 2 (n_win - 1) 2^-24) * rowmax_k,t as for daam_key_scores:
 *     |got - exact| <= sum_k |w_gk| e_k,t  +  c * 2^-24 * sum_k |w_gk * K_k[p]|
 * c = 2 + min(n_keys, 32) + (chunks > 1 ? chunks : 0), chunks = ceil(n_keys / 32): the product's rounding, K as an f32 value, the
 * additions inside a chunk of 32 keys and those of the join (tests/_blend_domain.py counts them).
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): 1 <= n_keys <= 2^20, 1 <= n_sets <= 8,
 * 1 <= out_h, out_w <= 128, 1 <= n_rows (and n_rows * bands of the output < 2^31, the launch grid), dtype one of the three, no
 * pointer NULL, set_stride >= n_rows * out_h * out_w, scratch_bytes >= daam_key_blend_scratch_bytes() of the same arguments.
 * DAAM_E_UNSUPPORTED when a workgroup's dynamic LDS would exceed 160 KB.
 *
 * Deterministic: no floating-point atomics.  Key k belongs to chunk k / 32; one workgroup owns a (token row, band of output rows,
 * chunk) and adds its keys of non-zero weight in key order, each lane into its own output elements; a second kernel adds the
 * chunks in which set g has a non-zero weight, in chunk order (a call of one chunk writes out itself).  The order in which keys
 * are added into an output element is therefore a fixed function of n_keys alone.  out[g] is bit-identical from run to run and
 * does not depend on the other sets of the call, on n_sets, on n_rows, on scratch_bytes or on where a plane starts in memory.
 * Rows at or past n_rows and bytes behind a plane are never read. */
DAAM_API int daam_key_blend(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, int out_h, int out_w,
                            const float* weights, int n_sets, float* out, int64_t set_stride, void* scratch, size_t scratch_bytes,
                            void* stream);
/* host only: bytes of scratch the call of the same arguments needs (0 when an argument is out of range); monotone in each */
DAAM_API size_t daam_key_blend_scratch_bytes(int n_keys, int n_sets, int n_rows, int out_h, int out_w);

DAAM_API int daam_blend_abi_version(void);             /* DAAM_BLEND_ABI_VERSION */
DAAM_API const char* daam_blend_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
