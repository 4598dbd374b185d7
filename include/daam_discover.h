/* daam_discover.h -- C ABI of libdaam_discover.so: segments from a self-affinity without a word list (DiffSeg-style discovery), on the
 * MI355X (gfx950).  Four stateless passes; `SelfAffinity.discover` (daam_amd/heatmap.py) strings them together, DESIGN 3.27 has the
 * arithmetic, its order and its error against float64.
 *
 *   prepare   rows of an affinity -> probability rows P and their logarithms L:
 *               s_r     = sum_j src[r][j] in ONE fixed order: thread t of 256 adds cells t, t + 256, t + 512, ... ascending into one
 *                         f32, the 256 partial sums are then added pairwise, partial[t] += partial[t + m] for m = 128, 64, ..., 1
 *               P[r][j] = src[r][j] / s_r                         (a correctly rounded f32 division)
 *               L[r][j] = logf(max(P[r][j], eps)), eps = 2^-120   (logf of the device library, not a fast intrinsic)
 *             a row whose sum is 0 or not finite gives P = 0 and L = logf(eps): no NaN is ever written.
 *   pair_kl   the symmetric KL divergence of A rows against B rows of N cells each:
 *               D[a][b] = 1/2 sum_j (Pa[a][j] - Pb[b][j]) * (La[a][j] - Lb[b][j])
 *             one accumulator per output, acc = fma(Pa - Pb, La - Lb, acc) with j ascending, halved at the end.  Every term is >= 0
 *             when L is the logarithm of P.  With Pa == Pb and La == Lb the diagonal is exactly 0 and D is bitwise symmetric.
 *   merge     out[k][j] = (sum over r ascending with member[k][r] != 0 of P[r][j]) / cnt_k, cnt_k the number of such r;
 *             cnt_k == 0 gives a row of zeros.
 *   labels    labels[y][x] = the lowest k at which the bilinear resize of props[k] to out_h x out_w is largest: the resize of
 *             F.interpolate(mode='bilinear', align_corners=False) with border-clamped taps, in f32; the source position
 *             ((2 y + 1) h - out_h) / (2 out_h) is formed in integers, so that with out == (h, w) every tap weight is exactly 1 or 0
 *             and the pass is a plain argmax.
 *
 * No atomics are used anywhere: every output element is written by exactly one workgroup, which adds in a fixed order; no result
 * depends on the grid and two runs give the same bits.  No kernel uses scratch.
 *
 * Conventions: those of daam_joint_affinity.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only
 * enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_discover_last_error() gives the message of the last failure on the calling
 * thread.  The library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing
 * from the other libraries but this header's include of daam_hip.h (DAAM_E_*).  Every limit below is checked on the host
 * (DAAM_E_INVALID with a message) before any HIP call; every pointer is 4-byte aligned unless it points to bytes; no output may
 * overlap an input or another output of the same call.
 */
#ifndef DAAM_DISCOVER_H
#define DAAM_DISCOVER_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_DISCOVER_ABI_VERSION 1

/* src f32 [R][N], row r at src + r * src_stride (elements; src_stride >= N), read-only.  P, L f32 [R][N], contiguous, overwritten in
 * full.  1 <= R <= 16384, 1 <= N <= 16384. */
DAAM_API int daam_discover_prepare(const float* src, int64_t src_stride, int R, int N, float* P, float* L, void* stream);

/* Pa, La f32 [A][N] and Pb, Lb f32 [B][N], contiguous, read-only (Pb may be Pa and Lb may be La).  D f32 [A][B], contiguous,
 * overwritten in full.  1 <= A, B <= 16384, 1 <= N <= 16384. */
DAAM_API int daam_discover_pair_kl(const float* Pa, const float* La, int A, const float* Pb, const float* Lb, int B, int N, float* D,
                                   void* stream);

/* P f32 [R][N] contiguous and member uint8 [K][R] contiguous, read-only.  out f32 [K][N] and cnt int32 [K], overwritten in full.
 * 1 <= R <= 16384, 1 <= N <= 16384, 1 <= K <= 1024. */
DAAM_API int daam_discover_merge(const float* P, int R, int N, const uint8_t* member, int K, float* out, int32_t* cnt, void* stream);

/* props f32 [K][h][w] contiguous, read-only.  labels uint8 [out_h][out_w], overwritten in full; values f32 [out_h][out_w], the
 * resized value of the winner, or NULL.  1 <= K <= 255, 1 <= h, w <= 128, 1 <= out_h, out_w <= 2048. */
DAAM_API int daam_discover_labels(const float* props, int K, int h, int w, int out_h, int out_w, uint8_t* labels, float* values,
                                  void* stream);

DAAM_API int daam_discover_abi_version(void);           /* DAAM_DISCOVER_ABI_VERSION */
DAAM_API const char* daam_discover_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
