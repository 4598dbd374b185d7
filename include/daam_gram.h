/* daam_gram.h -- C ABI of libdaam_gram.so: token co-attention on the MI355X (gfx950).
 *
 * daam_analysis.h answers which heads put a word on a region.  The pairwise question -- which heads and layers entangle two
 * words and which keep them apart, the reference's cohyponym / adjectival entanglement (daam/heatmap.py:95-96 through thresholded
 * masks of the GLOBAL map) -- has a threshold-free answer per (layer, head) key: the Gram matrix of the key's token planes, at
 * the key's own resolution, from the raw running sums (no bicubic, no clamp):
 *
 *   gram[k][i][j] = sum_p plane_k,i[p] * plane_k,j[p]                       i, j in [0, n_rows)
 *   cos[k][i][j]  = gram[k][i][j] / sqrt(gram[k][i][i] * gram[k][j][j] + eps)           (left to the caller)
 *
 * Word maps are means of token rows, so the Gram of two words is the mean of a block of gram[k], exactly: one matrix per key
 * answers every word pair.
 *
 * Conventions: those of daam_hip.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t passed as
 * void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_gram_last_error() gives the message of the last
 * failure on the calling thread.  The library holds no context and no state between calls, and works on the HIP device that is
 * current.  It is separate from libdaam_hip.so and libdaam_analysis.so and needs nothing from them but this header's include of
 * daam_analysis.h (DaamKeyPlanes, and through it the DAAM_E_* and dtype codes).
 */
#ifndef DAAM_GRAM_H
#define DAAM_GRAM_H

#include "daam_analysis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_GRAM_ABI_VERSION 1

/* Per-key Gram matrices.  `keys` [n_keys] on the device (DaamKeyPlanes of daam_analysis.h: base, win_stride, h, w, n_win keep their
 * meaning; only h * w matters here -- planes are [>= n_rows][h * w], contiguous, at any element alignment); `dtype` (DAAM_F16 |
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
DAAM_API int daam_gram_abi_version(void);              /* DAAM_GRAM_ABI_VERSION */
DAAM_API const char* daam_gram_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
