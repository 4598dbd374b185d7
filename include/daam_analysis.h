/* daam_analysis.h -- C ABI of libdaam_analysis.so: per-key analyses on the MI355X (gfx950).
 *
 * Head analysis.  The reference gives DiffusionHeatMapHooker.compute_global_heat_map its head_idx= / layer_idx= arguments
 * (daam/trace.py:103-126) so that one can ask which heads and layers carry a word: per selected (factor, layer, head)
 * key the running sum is resized to the map's size (bicubic), clamped at 0 and -- for a score -- weighed inside an image
 * region, which is what WordHeatMap.expand_as(absolute=True) (daam/heatmap.py:77-93) followed by a masked sum gives.
 * The clamp sits between the bicubic and the sum over keys, so per-key scores cannot be taken from the global map;
 * daam_key_scores computes them from ONE read of the running sums, without writing a map per key:
 *
 *   scores[k][m][t] = sum_p footprint[m][p] * max(bicubic(plane_k,t -> out_h x out_w)[p], 0)        t in [0, n_rows)
 *
 * Token co-attention.  The pairwise question -- which heads and layers entangle two words and which keep them apart, the
 * reference's cohyponym / adjectival entanglement (daam/heatmap.py:95-96 through thresholded masks of the GLOBAL map) -- has a
 * threshold-free answer per (layer, head) key: the Gram matrix of the key's token planes, at the key's own resolution, from the
 * raw running sums (no bicubic, no clamp), which daam_token_gram computes:
 *
 *   gram[k][i][j] = sum_p plane_k,i[p] * plane_k,j[p]                       i, j in [0, n_rows)
 *   cos[k][i][j]  = gram[k][i][j] / sqrt(gram[k][i][i] * gram[k][j][j] + eps)           (left to the caller)
 *
 * Word maps are means of token rows, so the Gram of two words is the mean of a block of gram[k], exactly: one matrix per key
 * answers every word pair.
 *
 * Key blend.  The two above say WHICH keys matter; daam_key_blend makes the map of a chosen set of them.  It is the finalize's
 * arithmetic (compute_global_heat_map, reference daam/trace.py:116-126) with a weight per key in front of the sum over keys, for
 * up to 8 weight sets from ONE read of the running sums:
 *
 *   out[g][t][p] = sum_k  w[g][k] * max(bicubic(plane_k,t -> out_h x out_w)[p], 0)        t in [0, n_rows),  g in [0, n_sets)
 *
 * Again the clamp sits between the bicubic and the sum over keys, so this cannot be derived from the global map or from per-key
 * scores.  With w = 1 / n_keys it is the global heat map of the same keys.
 *
 * Conventions: those of daam_hip.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t
 * passed as void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_analysis_last_error() gives the
 * message of the last failure of any of the calls on the calling thread.  The library holds no context and no state between calls,
 * and works on the HIP device that is current.  It is separate from libdaam_hip.so and needs nothing from it but this header's
 * include of daam_hip.h (the DAAM_E_* and dtype codes).
 */
#ifndef DAAM_ANALYSIS_H
#define DAAM_ANALYSIS_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_ANALYSIS_ABI_VERSION 3

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

/* Per-key Gram matrices.  `keys` [n_keys] on the device (base, win_stride, h, w, n_win keep their meaning; only h * w matters
 * here -- planes are [>= n_rows][h * w], contiguous, at any element alignment); `dtype` (DAAM_F16 |
 * DAAM_F32 | DAAM_BF16) is the planes' element type; `gram` [n_keys][n_rows][n_rows] fp32 is overwritten in full.  n_win > 1: the
 * windows' planes are added in f32, in window order, BEFORE the products -- the Gram of a generation that ran exactly those steps.
 *
 * `scratch` holds the partial matrices of keys of more than 1024 pixels: daam_token_gram_scratch_bytes(n_keys, n_rows, max_hw)
 * bytes serve every key of up to max_hw pixels.  The call takes the chunks per key it may use from scratch_bytes; a key of more
 * pixels than that allows is not read and its matrix is NaN, like a key whose h, w (1..128) or n_win (>= 1) is out of range.
 *
 * Arithmetic.  A key's pixels are cut into chunks of 1024; one workgroup of four waves owns a (key, chunk).
 *   16-bit planes with n_win == 1: the planes' own bits are the operands of v_mfma_f32_32x32x16_f16 / _bf16 (products exact in
 *     f32, fp16 subnormals included; bf16 products must not underflow f32).  A sub-tile of 128 pixels is 8 k-steps; wave v takes
 *     k-steps 2v and 2v + 1 of every sub-tile.
 *   f32 planes, and any n_win > 1: widened, windows added, then v_mfma_f32_32x32x2_f32 (a k-ordered fused multiply-add chain);
 *     a sub-tile of 64 pixels is 32 k-steps, wave v takes 8v .. 8v + 7.
 *   The four waves are joined as (w0 + w1) + (w2 + w3); a second kernel adds a key's chunks in chunk order (a one-chunk key is
 *   written by the first kernel: adding nothing changes no bit).  Only the blocks on and above the diagonal of the matrix of
 *   32 x 32 blocks are computed; every element below the diagonal is a copy of its mirror.
 * Error, with c = the longest chain of f32 additions (tests/_gram_domain.py counts it: 16 per 16-bit k-step or 2 per f32 k-step of
 * a wave, 2 for the waves, chunks - 1), each allowed 2^-23:
 *     |got - exact| <= c * 2^-23 * sum_p |a_i[p] * a_j[p]|        (+ 2^-24 per product on the f32 path, + the windows' additions:
 *     2 (n_win - 1) 2^-24 max |partial sum| per element, carried through the product)
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): 1 <= n_keys <= 2^20, 1 <= n_rows <= 96, dtype one of
 * the three, keys / gram / scratch not NULL, scratch_bytes >= daam_token_gram_scratch_bytes(n_keys, n_rows, 1).
 *
 * Deterministic: no floating-point atomics.  gram[k] is bit-identical from run to run, does not depend on the other keys of the
 * call, on n_keys, on scratch_bytes or on where a plane starts in memory, and is bitwise symmetric.  Rows at or past n_rows and
 * bytes behind a plane are never read. */
DAAM_API int daam_token_gram(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, float* gram, void* scratch,
                             size_t scratch_bytes, void* stream);
/* host only: bytes of scratch that serve n_keys keys of up to max_hw pixels each (0 when an argument is out of range); monotone */
DAAM_API size_t daam_token_gram_scratch_bytes(int n_keys, int n_rows, int max_hw);

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

DAAM_API int daam_analysis_abi_version(void);          /* DAAM_ANALYSIS_ABI_VERSION */
DAAM_API const char* daam_analysis_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
