/* daam_self_affinity.h -- C ABI of libdaam_selfaff.so: the self-attention affinity of a generation and the propagation of soft word
 * maps along it, on the MI355X (gfx950).
 *
 * The semantic affinity between two cells of the heat map's grid sits in the UNet that is already hooked: the self-attention (attn1)
 * of the transformer blocks whose cross-attention is tapped.  Averaged over heads, layers and steps it is a P x P matrix (P = h w
 * cells) along which a cross-attention word map is spread (DiffSegmenter, iSeg, Dataset-Diffusion and kin).  The contract:
 *
 *   q, k          fp16 or bf16 (DAAM_F16 / DAAM_BF16), seen as [batch][heads][P][d]; d is contiguous, the batch, head and row strides
 *                 are given in ELEMENTS, so that what to_q / to_k produce, [batch, P, heads d], and a packed [batch, heads, P, d]
 *                 are both read without a copy.  A slice is s = b * heads + h, S = batch * heads of them.
 *   logits        x_s[i][j] = scale * sum_c q_s[i][c] k_s[j][c]
 *   probabilities p_s[i][.] = softmax_j x_s[i][.], the row maximum subtracted
 *   accumulator   acc[i][j] = sum_s p_s[i][j], s ascending
 *   sums          sums[i][j] = fma(weight, acc[i][j], accumulate ? sums[i][j] : 0), f32 [P][P]
 *
 *   propagation   r_i = sum_j sums[i][j];  m^{t+1}_n(i) = (sum_j sums[i][j] m^t_n(j)) / r_i, a row with r_i == 0 keeps m^t_n(i);
 *                 refined = m^T, T = 0 copies the input's bits.
 *
 * The logits stay in f32 as they leave the MFMA accumulators: they are NOT rounded to the input dtype.  This is an analysis
 * quantity, not a replay of the model's own arithmetic (the model's output is untouched by it).
 * No atomics are used anywhere: every element of sums is written by exactly one workgroup, which adds the slices in ascending order
 * in registers; no result depends on the grid and two runs give the same bits.  The arithmetic, its order and its error against
 * float64 are in DESIGN 3.22.
 *
 * Conventions: those of daam_refine.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only enqueue,
 * 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_self_affinity_last_error() gives the message of the last failure on the calling
 * thread.  The library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing
 * from the other libraries but this header's include of daam_hip.h (DAAM_E_*, DAAM_F16, DAAM_BF16).
 */
#ifndef DAAM_SELF_AFFINITY_H
#define DAAM_SELF_AFFINITY_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_SELF_AFFINITY_ABI_VERSION 1

/* host only; 0 = out of range.  The scratch of daam_self_affinity_accumulate, a multiple of 8: the softmax statistics (-max, 1 / sum)
 * of every row of every slice, rows padded to whole tiles.  batch, heads >= 1, batch * heads <= 4096, 1 <= P <= 16384. */
DAAM_API size_t daam_self_affinity_workspace(int batch, int heads, int P);
/* host only; 0 = out of range.  The scratch of daam_self_affinity_propagate, a multiple of 8: one stack of maps f32 [N][P] that the
 * iterations alternate with `refined`, and the row sums f32 [P].  1 <= N <= 32, 1 <= P <= 16384. */
DAAM_API size_t daam_self_affinity_propagate_workspace(int N, int P);

/* q, k: 16-byte aligned, read-only; every stride >= 0 and a multiple of 8 elements (16-byte rows, the rule of the strided tap ABI),
 * the row strides >= d.  in_dtype DAAM_F16 or DAAM_BF16.  d in {40, 64, 80, 160}.  scale finite and > 0, weight finite.
 * sums f32 [P][P], 4-byte aligned: with accumulate == 0 its previous bytes are never read and every element is overwritten.
 * workspace: at least daam_self_affinity_workspace(batch, heads, P) bytes, 8-byte aligned, the caller's between calls; besides sums it
 * is the only memory written; it must not overlap sums.  Two launches: the statistics, then the sums.
 * Every limit is checked on the host (DAAM_E_INVALID with a message) before any HIP call. */
DAAM_API int daam_self_affinity_accumulate(const void* q, const void* k, int in_dtype, int batch, int heads, int P, int d,
                                           int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p, int64_t k_stride_b,
                                           int64_t k_stride_h, int64_t k_stride_p, float scale, float weight, int accumulate, float* sums,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* sums f32 [P][P] and maps f32 [N][P], read-only, 4-byte aligned.  The entries of sums must be finite and >= 0: that is the CALLER'S
 * duty (what daam_self_affinity_accumulate leaves with weights >= 0 is).  1 <= N <= 32, 0 <= iterations <= 16.
 *   refined [N][P] f32, overwritten in full; with iterations == 0 the bits of maps
 * One launch per iteration (the first also forms the row sums, in the same pass, and leaves them in the workspace); a launch serves
 * all N maps of a row, so every element of sums is fetched once per iteration.  Summation order: lane l of the row's wave adds the
 * terms j = l, l + 64, ... ascending, the 64 partial sums are combined by a butterfly over the lane distances 32, 16, 8, 4, 2, 1;
 * then one IEEE division.
 * workspace: at least daam_self_affinity_propagate_workspace(N, P) bytes, 4-byte aligned.  What is written (refined, the workspace)
 * must overlap nothing that is read (sums, maps) nor each other: refined against maps, sums and the workspace, the workspace against
 * maps and sums (host-checked). */
DAAM_API int daam_self_affinity_propagate(const float* sums, int P, const float* maps, int N, int iterations, float* refined,
                                          void* workspace, size_t workspace_bytes, void* stream);

DAAM_API int daam_self_affinity_abi_version(void);            /* DAAM_SELF_AFFINITY_ABI_VERSION */
DAAM_API const char* daam_self_affinity_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
