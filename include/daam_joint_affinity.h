/* daam_joint_affinity.h -- C ABI of libdaam_jointaff.so: the image-to-image block of the joint attention of an MMDiT / FLUX block,
 * summed over slices into one affinity matrix, on the MI355X (gfx950).
 *
 * An MMDiT block has no self-attention of its own: the image tokens attend to text AND image keys in one softmax.  The affinity of
 * image cell i to image cell j is the probability p[i][j] of that joint softmax for image key j, with the text keys in the
 * denominator.  This library does NOT form the softmax statistics: it reads them, one (shift, reciprocal) pair per query row, and
 * recomputes only the image columns.  The contract:
 *
 *   q, k_img      the image queries and image keys, fp16 or bf16 (DAAM_F16 / DAAM_BF16), seen as [batch][heads][P][d] and
 *                 [batch][heads][Pk][d]; d is contiguous, the batch, head and row strides are given in ELEMENTS, so that what the
 *                 projections produce, [batch, rows, heads d], and a packed [batch, heads, rows, d] are both read without a copy.
 *                 A slice is s = b * heads + h, S = batch * heads of them.
 *   stats         float2 per query row, read-only: element s * pad128(P) + i is (-(m_i c), 1 / l_i) of row i of slice s, where
 *                 pad128(P) is P rounded up to a multiple of 128, c = f32(scale * log2(e)) (the double product rounded once),
 *                 m_i the maximum of the raw dot products raw_s[i][.] = sum_c q_s[i][c] k_s[.][c] over ALL keys of the row's
 *                 softmax (text keys included) and l_i = sum over all those keys of exp2(fma(raw, c, -(m_i c))).  This is what
 *                 daam_joint_tap_accumulate of DAAM_JOINT_TAP_ABI_VERSION 1 leaves in its workspace after a call on the same q,
 *                 k_txt, k_img, scale; statistics from anywhere else in this layout serve as well.  Only rows i < P are read.
 *   probabilities p_s[i][j] = exp2(fma(raw_s[i][j], c, stats.x)) * stats.y for image key j, raw in f32 as it leaves the MFMA
 *                 accumulators (NOT rounded to the input dtype)
 *   accumulator   acc[i][j] = sum_s p_s[i][j], s ascending
 *   sums          sums[i][j] = fma(weight, acc[i][j], accumulate ? sums[i][j] : 0), f32 [P][Pk], contiguous, query-major (with
 *                 Pk == P the layout of the sums of daam_self_affinity.h)
 *
 * A row of acc sums to S minus the mass the cell gave to the text keys.  One launch.  No atomics are used anywhere: every element
 * of sums is written by exactly one workgroup, which adds its slices in ascending order in registers; no result depends on the grid
 * and two runs give the same bits.  The arithmetic, its order and its error against float64 are in DESIGN 3.26.
 *
 * Conventions: those of daam_joint_tap.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only enqueue,
 * 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_joint_affinity_last_error() gives the message of the last failure on the calling
 * thread.  The library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing
 * from the other libraries but this header's include of daam_hip.h (DAAM_E_*, DAAM_F16, DAAM_BF16).
 */
#ifndef DAAM_JOINT_AFFINITY_H
#define DAAM_JOINT_AFFINITY_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_JOINT_AFFINITY_ABI_VERSION 1

/* host only; 0 = out of range.  The bytes of the statistics of batch * heads slices of P rows: 8 * batch * heads * pad128(P).
 * batch, heads >= 1, batch * heads <= 4096, 1 <= P <= 16384. */
DAAM_API size_t daam_joint_affinity_stats_bytes(int batch, int heads, int P);

/* q, k_img: 16-byte aligned, read-only; every stride >= 0 and a multiple of 8 elements (16-byte rows), the row strides >= d.
 * in_dtype DAAM_F16 or DAAM_BF16.  1 <= P, Pk <= 16384, d in {64, 128}, batch * heads <= 4096.  scale finite and > 0 (the scale the
 * statistics were formed with), weight finite.
 * stats: 8-byte aligned, read-only, stats_bytes >= daam_joint_affinity_stats_bytes(batch, heads, P); it must not overlap sums.
 * sums f32, 4-byte aligned, the only memory written: with accumulate == 0 its previous bytes are never read and every element is
 * overwritten.
 * Every limit is checked on the host (DAAM_E_INVALID with a message) before any HIP call. */
DAAM_API int daam_joint_affinity_accumulate(const void* q, const void* k_img, const void* stats, size_t stats_bytes, int in_dtype,
                                            int batch, int heads, int P, int Pk, int d, int64_t q_stride_b, int64_t q_stride_h,
                                            int64_t q_stride_p, int64_t ki_stride_b, int64_t ki_stride_h, int64_t ki_stride_p,
                                            float scale, float weight, int accumulate, float* sums, void* stream);

DAAM_API int daam_joint_affinity_abi_version(void);           /* DAAM_JOINT_AFFINITY_ABI_VERSION */
DAAM_API const char* daam_joint_affinity_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
