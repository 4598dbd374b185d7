/* daam_joint_attend.h -- C ABI of libdaam_jointattend.so: the joint attention of an MMDiT block (Stable Diffusion 3 class) itself,
 * softmax(Q K^T) V for the image AND the text queries over text and image keys, with the image rows' softmax statistics left behind
 * as a by-product of the one key walk, on the MI355X (gfx950); and the text columns of that softmax from given statistics.
 *
 * With this library a traced block computes its attention once: the model's output and the (shift, reciprocal) pair of every image
 * row come from the same walk, and the heat-map planes (and, with the affinity, the image columns: daam_joint_affinity.h) cost their
 * small second kernels and nothing more.  The contract of daam_joint_attend_forward:
 *
 *   q_img, k_img, v_img   fp16 or bf16 (DAAM_F16 / DAAM_BF16), seen as [batch][heads][P][d]
 *   q_txt, k_txt, v_txt   seen as [batch][heads][T][d]; d is contiguous, every tensor has its own batch, head and row strides in
 *                         ELEMENTS, so that what the projections produce, [batch, rows, heads d], and a packed [batch, heads, rows, d]
 *                         are both read without a copy: no concatenation, no transpose.  A slice is s = b * heads + h, S of them.
 *   logits                x_s[i][j] = scale * sum_c q_s[i][c] k_s[j][c] over all T + P keys, for every query row i of either kind;
 *                         they stay in f32 as they leave the MFMA accumulators
 *   probabilities         p_s[i][.] = softmax over ALL T + P keys, the row maximum subtracted
 *   out_img, out_txt      o_s[i][c] = sum_j p_s[i][j] v_s[j][c], rounded ONCE to the input dtype, through strides of the same kind; a
 *                         convex combination: V up to the dtype's largest finite value gives no Inf on the way;
 *                         only the d elements of a row are written: bytes between rows are left alone
 *   stats                 NULL (nothing is written), or float2 per IMAGE query row: element s * pad128(P) + i receives
 *                         (-(m_i c), 1 / l_i), pad128(P) = P rounded up to a multiple of 128, c = f32(scale * log2(e)) (the double
 *                         product rounded once), m_i the maximum of the raw dot products over all keys and
 *                         l_i = sum over all keys of exp2(fma(raw, c, -(m_i c))): the layout and the meaning of what
 *                         daam_joint_tap_accumulate (ABI 1) leaves in its workspace and daam_joint_affinity_accumulate reads.
 *                         Rows P .. pad128(P) - 1 of a slice are written too (the statistics of an all-zero query).  The
 *                         statistics of the text queries do not leave the kernel.
 *
 * daam_joint_attend_text computes the text columns from given statistics: word for word the second launch of
 * daam_joint_tap_accumulate --
 *
 *   accumulator   sums_stride_h == 0:     one plane, acc[t][i] = sum_s p_s[i][t], s ascending,
 *                                         p_s[i][t] = exp2(fma(raw_s[i][t], c, stats.x)) * stats.y
 *                 sums_stride_h >= T * P: `heads` planes sums_stride_h floats apart; plane h takes the slices with s mod heads == h,
 *                                         batch ascending
 *   sums          sums[t][i] = fma(weight, acc[t][i], accumulate ? sums[t][i] : 0), f32 [T][P]: token-major, cells contiguous
 *
 * with the statistics read-only, as in daam_joint_affinity_accumulate.  A caller that taps the kept half of a batch passes q_img and
 * k_txt offset to batch `first`, stats + first * heads * pad128(P) and batch - first.
 *
 * One launch each.  No atomics are used anywhere and the library holds no state: every output element is written by exactly one
 * workgroup, slices are added in ascending order in registers, no result depends on the grid and two runs give the same bits.  The
 * arithmetic, its order and its error against float64 are in DESIGN 3.28.
 *
 * Conventions: those of daam_joint_tap.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only enqueue,
 * 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_joint_attend_last_error() gives the message of the last failure on the calling
 * thread.  The library works on the HIP device that is current.  It needs nothing from the other libraries but this header's include
 * of daam_hip.h (DAAM_E_*, DAAM_F16, DAAM_BF16).
 */
#ifndef DAAM_JOINT_ATTEND_H
#define DAAM_JOINT_ATTEND_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_JOINT_ATTEND_ABI_VERSION 1

/* host only; 0 = out of range.  The bytes of the statistics of batch * heads slices of P rows: 8 * batch * heads * pad128(P), the
 * layout daam_joint_affinity.h states.  batch, heads >= 1, batch * heads <= 4096, 1 <= P <= 16384. */
DAAM_API size_t daam_joint_attend_stats_bytes(int batch, int heads, int P);

/* The six inputs: 16-byte aligned, read-only.  out_img, out_txt: 16-byte aligned, of in_dtype.  Every stride >= 0 and a multiple of
 * 8 elements (16-byte rows), the row strides >= d; the output strides are such that no two rows of an output share an element:
 * with heads > 1 either stride_h >= (rows - 1) stride_p + d (rows inside a head) or stride_h >= d and stride_p >= (heads - 1) stride_h
 * + d (heads inside a row), and with batch > 1 stride_b >= (heads - 1) stride_h + (rows - 1) stride_p + d.
 * in_dtype DAAM_F16 or DAAM_BF16.  1 <= P <= 16384, 1 <= T <= 512, d in {64, 128}, batch * heads <= 4096.  scale finite and > 0.
 * stats: NULL, or 8-byte aligned with stats_bytes >= daam_joint_attend_stats_bytes(batch, heads, P); it must not overlap an output.
 * Every limit is checked on the host (DAAM_E_INVALID with a message) before any HIP call. */
DAAM_API int daam_joint_attend_forward(const void* q_img, const void* k_img, const void* v_img, const void* q_txt, const void* k_txt,
                                       const void* v_txt, void* out_img, void* out_txt, int in_dtype, int batch, int heads, int P, int T,
                                       int d, const int64_t* img_strides, const int64_t* txt_strides, const int64_t* out_strides,
                                       float scale, void* stats, size_t stats_bytes, void* stream);
/* img_strides: 9 numbers, (batch, head, row) of q_img, k_img, v_img in that order; txt_strides: the same of q_txt, k_txt, v_txt;
 * out_strides: 6 numbers, (batch, head, row) of out_img and of out_txt.  The arrays are read on the host during the call. */

/* q_img, k_txt: 16-byte aligned, read-only; the six strides are (batch, head, row) of q_img and of k_txt, as above.
 * stats: 8-byte aligned, READ-ONLY, stats_bytes >= daam_joint_attend_stats_bytes(batch, heads, P); it must not overlap sums.
 * scale: the scale the statistics were formed with; weight finite.  sums_stride_h (in floats): 0, or >= T * P.
 * sums f32, 4-byte aligned, the only memory written: with accumulate == 0 its previous bytes are never read and every element of
 * every plane is overwritten (with heads planes the floats between two planes are not touched). */
DAAM_API int daam_joint_attend_text(const void* q_img, const void* k_txt, const void* stats, size_t stats_bytes, int in_dtype, int batch,
                                    int heads, int P, int T, int d, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p,
                                    int64_t kt_stride_b, int64_t kt_stride_h, int64_t kt_stride_t, float scale, float weight,
                                    int accumulate, float* sums, int64_t sums_stride_h, void* stream);

DAAM_API int daam_joint_attend_abi_version(void);             /* DAAM_JOINT_ATTEND_ABI_VERSION */
DAAM_API const char* daam_joint_attend_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
