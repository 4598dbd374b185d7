/* daam_joint_tap.h -- C ABI of libdaam_joint.so: the image-to-text block of the joint attention of an MMDiT block (Stable Diffusion 3
 * class), summed over slices into a heat-map plane, on the MI355X (gfx950).
 *
 * In an MMDiT block the image tokens attend to text AND image keys in one softmax.  The DAAM quantity is the probability an image
 * cell gives to a text token, with the image keys in the denominator.  The contract:
 *
 *   q             the image queries, fp16 or bf16 (DAAM_F16 / DAAM_BF16), seen as [batch][heads][P][d]
 *   k_txt, k_img  the text and image keys, [batch][heads][T][d] and [batch][heads][Pk][d]; d is contiguous, the batch, head and row
 *                 strides are given in ELEMENTS, so that what the projections produce, [batch, rows, heads d], and a packed
 *                 [batch, heads, rows, d] are both read without a copy.  A slice is s = b * heads + h, S = batch * heads of them.
 *   logits        x_s[i][j] = scale * sum_c q_s[i][c] k_s[j][c] over the T + Pk keys (their order is immaterial)
 *   probabilities p_s[i][.] = softmax over ALL T + Pk keys, the row maximum subtracted; only the T text columns leave the kernel
 *   accumulator   sums_stride_h == 0:     one plane, acc[t][i] = sum_s p_s[i][t], s ascending
 *                 sums_stride_h >= T * P: `heads` planes sums_stride_h floats apart; plane h takes the slices with s mod heads == h,
 *                                         batch ascending
 *   sums          sums[t][i] = fma(weight, acc[t][i], accumulate ? sums[t][i] : 0), f32 [T][P]: token-major, cells contiguous (the
 *                 layout of a heat map)
 *
 * Pk == 0 is the text-only softmax of a UNet's cross-attention, a legal degenerate case (k_img is then not read and may be NULL).
 * The logits stay in f32 as they leave the MFMA accumulators: they are NOT rounded to the input dtype (a fused SDPA does not round
 * them either).  No atomics are used anywhere: every element of sums is written by exactly one workgroup, which adds its slices in
 * ascending order in registers; no result depends on the grid and two runs give the same bits.  The arithmetic, its order and its
 * error against float64 are in DESIGN 3.24.
 *
 * Conventions: those of daam_self_affinity.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only
 * enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_joint_tap_last_error() gives the message of the last failure on the calling
 * thread.  The library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing
 * from the other libraries but this header's include of daam_hip.h (DAAM_E_*, DAAM_F16, DAAM_BF16).
 */
#ifndef DAAM_JOINT_TAP_H
#define DAAM_JOINT_TAP_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_JOINT_TAP_ABI_VERSION 1

/* host only; 0 = out of range.  The scratch of daam_joint_tap_accumulate, a multiple of 8: the softmax statistics (-max, 1 / sum) of
 * every query row of every slice, rows padded to whole blocks.  batch, heads >= 1, batch * heads <= 4096, 1 <= P <= 16384. */
DAAM_API size_t daam_joint_tap_workspace(int batch, int heads, int P);

/* q, k_txt, k_img: 16-byte aligned, read-only; every stride >= 0 and a multiple of 8 elements (16-byte rows), the row strides >= d.
 * in_dtype DAAM_F16 or DAAM_BF16.  1 <= P <= 16384, 1 <= T <= 512, 0 <= Pk <= 16384, d in {64, 128}, batch * heads <= 4096.
 * scale finite and > 0, weight finite.  sums_stride_h (in floats): 0, or >= T * P.
 * sums f32, 4-byte aligned: with accumulate == 0 its previous bytes are never read and every element of every plane is overwritten
 * (with heads planes the floats between two planes are not touched).
 * workspace: at least daam_joint_tap_workspace(batch, heads, P) bytes, 8-byte aligned, the caller's between calls; besides sums it is
 * the only memory written; it must not overlap sums.  Two launches: the statistics, then the text columns.
 * Every limit is checked on the host (DAAM_E_INVALID with a message) before any HIP call. */
DAAM_API int daam_joint_tap_accumulate(const void* q, const void* k_txt, const void* k_img, int in_dtype, int batch, int heads, int P,
                                       int T, int Pk, int d, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p,
                                       int64_t kt_stride_b, int64_t kt_stride_h, int64_t kt_stride_t, int64_t ki_stride_b,
                                       int64_t ki_stride_h, int64_t ki_stride_p, float scale, float weight, int accumulate,
                                       float* sums, int64_t sums_stride_h, void* workspace, size_t workspace_bytes, void* stream);

DAAM_API int daam_joint_tap_abi_version(void);                /* DAAM_JOINT_TAP_ABI_VERSION */
DAAM_API const char* daam_joint_tap_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
