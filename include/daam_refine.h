/* daam_refine.h -- C ABI of libdaam_refine.so: image-guided refinement of soft word maps on the MI355X (gfx950).
 *
 * Local-affinity propagation.  A word mask is a bicubic blow-up of a 64 x 64 (or smaller) attention map: a blob that ignores the
 * object's outline.  The remedy is to propagate the soft map along the generated image's own local colour affinities for a few
 * iterations (pixel-adaptive refinement, the cheap stand-in for a dense CRF).  The contract:
 *
 *   image I       uint8 [h][w][c], c in {1, 3}, values taken as I / 255
 *   dilations D   d_1 < ... < d_n, 1 <= n <= 6, 1 <= d <= 64
 *   scale s       finite, > 0
 *   maps m^0      f32 [n_maps][h][w], finite
 *
 *   neighbours    q_k(p), k = 0 .. K - 1, K = 8 n, of the pixel p = (y, x): dilation-major, then the eight offsets
 *                 (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1) times d as (dy, dx); each coordinate is clamped to the image
 *                 (replicate border).
 *   deviation     sigma_c(p) = the population standard deviation of channel c over the K + 1 samples {I_c(q_k(p))} and I_c(p).
 *   weights       a_k(p) = -(1/c) sum_c |I_c(q_k(p)) - I_c(p)| / (1e-8 + s sigma_c(p)),  w_k(p) = softmax_k a_k(p) with the maximum
 *                 subtracted.  They depend on the image alone: daam_refine_affinity computes them once, daam_refine_apply reuses
 *                 them for every map and every iteration.
 *   iteration     m^{t+1}_j(p) = sum_k w_k(p) m^t_j(q_k(p)),  t = 0 .. T - 1;  T = 0 copies the input.
 *   outputs       refined = m^T;  masks[j][p] = refined_j(p) > threshold as 0 / 1;  labels[p] = the smallest j that attains
 *                 max_j refined_j(p) when that maximum is > threshold, else 255 (the rule of daam_word_masks).
 *
 * Every step is a convex combination, so refined stays inside [min m^0, max m^0] (up to f32 rounding); the maps are not
 * renormalised afterwards.  No atomics are used anywhere and no result depends on the grid: two runs give the same bits.
 * The arithmetic, its order and its error against float64 are in DESIGN 3.21.
 *
 * Conventions: those of daam_components.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t passed
 * as void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_refine_last_error() gives the message of the last
 * failure on the calling thread.  The library holds no context and no state between calls, and works on the HIP device that is
 * current.  It needs nothing from the other libraries but this header's include of daam_hip.h (DAAM_E_*).
 */
#ifndef DAAM_REFINE_H
#define DAAM_REFINE_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_REFINE_ABI_VERSION 1

/* host only; 0 = out of range.  The bytes of the weight tensor, f32 [K = 8 n_dil][h][w]:  1 <= n_dil <= 6, h, w >= 1,
 * K h w < 2^31. */
DAAM_API size_t daam_refine_weights_bytes(int h, int w, int n_dil);
/* host only; 0 = out of range.  The scratch of daam_refine_apply, a multiple of 8: one plane stack f32 [n_maps][h][w] that the
 * iterations alternate with `refined`.  1 <= n_maps <= 32, h, w >= 1, 8 h w < 2^31. */
DAAM_API size_t daam_refine_workspace(int n_maps, int h, int w);

/* image [h][w][channels] uint8, contiguous at any byte alignment, read-only.  dilations: HOST array of n_dil ints.
 * weights [8 n_dil][h][w] f32 (4-byte aligned), overwritten in full: weights[k][y][x] = w_k((y, x)).  One launch; per pixel the
 * sums behind sigma are exact integers. */
DAAM_API int daam_refine_affinity(const uint8_t* image, int h, int w, int channels, const int32_t* dilations, int n_dil,
                                  float scale, float* weights, void* stream);

/* weights as daam_refine_affinity leaves them for the same h, w and dilations (HOST array); maps [n_maps][h][w] f32; both
 * read-only.  0 <= iterations <= 64.  threshold finite (unused when masks and labels are both NULL).
 *   refined [n_maps][h][w] f32      m^T; with iterations == 0 the bits of maps
 *   masks   [n_maps][h][w] uint8 or NULL, at any byte alignment
 *   labels  [h][w] uint8 or NULL, at any byte alignment
 * All outputs are overwritten in full.  One launch per iteration (an iteration reads a halo of up to 64 pixels of the one before:
 * a global dependency); a launch handles all n_maps maps of a pixel, so every weight is fetched once per iteration; the last
 * launch writes refined, masks and labels together: there is no extra pass at image resolution.
 * workspace: at least daam_refine_workspace(n_maps, h, w) bytes, 4-byte aligned, the caller's between calls; besides the outputs it
 * is the only memory written.  refined must overlap neither maps nor the workspace.
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): those above; dilations strictly increasing within
 * 1 .. 64; scale finite and > 0; no NULL among image / weights / dilations / maps / refined / workspace. */
DAAM_API int daam_refine_apply(const float* weights, const int32_t* dilations, int n_dil, const float* maps, int n_maps, int h, int w,
                               int iterations, float threshold, float* refined, uint8_t* masks, uint8_t* labels, void* workspace,
                               size_t workspace_bytes, void* stream);

DAAM_API int daam_refine_abi_version(void);            /* DAAM_REFINE_ABI_VERSION */
DAAM_API const char* daam_refine_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
