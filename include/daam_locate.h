/* daam_locate.h -- C ABI of libdaam_locate.so: localisation of words on the MI355X (gfx950).
 *
 * Boxes, peaks and pointing hits.  Two localisation measures are taken from attribution maps besides mask overlap: the bounding
 * box of a word -- the box of the mask WordHeatMap.expand_as(image, threshold=tau) (reference daam/heatmap.py:77-93) gives,
 * scored by box IoU against a truth box (CorLoc) -- and the pointing game -- whether the peak of the word's map falls inside the
 * object's mask.  Let v_j(p) be what daam_word_masks compares with its threshold.  The mask of word j at tau is v_j(p) > tau,
 * so row y holds a mask pixel iff max_x v_j(y, x) > tau, and column x iff max_y v_j(y, x) > tau: the box at EVERY tau follows
 * from the out_h row maxima and the out_w column maxima.  The min-max normalisation q(v) = (v - lo) / (hi - lo + 1e-8f) of
 * heatmap.py:84-85 is non-decreasing in v in f32 (a correctly rounded subtraction of a constant is monotone, and so is the
 * division by a positive constant), hence max q(v) = q(max v) and the maxima are taken on the raw resized values.  One pass at
 * image resolution gives, per word, the out_h + out_w maxima, lo, hi and the arg-max; nothing is written at image resolution.
 *
 * Conventions: those of daam_eval.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t passed as
 * void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_locate_last_error() gives the message of the last
 * failure on the calling thread.  The library holds no context and no state between calls, and works on the HIP device that is
 * current.  It needs nothing from the other libraries but this header's include of daam_hip.h (DAAM_E_*).
 */
#ifndef DAAM_LOCATE_H
#define DAAM_LOCATE_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_LOCATE_ABI_VERSION 1

/* word_maps [n_words][h][w] fp32: the un-expanded mean planes, as daam_word_masks leaves them; 0 <= n_words <= 32 (NULL iff
 *   n_words == 0), 1 <= h, w <= 128.  The planes must be finite: what a NaN or an infinity does is not specified.
 * thresholds: HOST array of n_thr finite floats, 0 <= n_thr <= 64 (may be NULL when n_thr == 0), in any order, duplicates
 *   allowed: each is handled on its own.
 * truth [n_truth][out_h][out_w] uint8 (a byte != 0 is set; contiguous planes at any byte alignment), 0 <= n_truth <= 32 (NULL iff
 *   n_truth == 0).  n_words + n_truth >= 1.  out_h, out_w >= 1, out_h * out_w < 2^31.
 *
 * v_j(p) := what daam_word_masks compares with its threshold for word j at pixel p under the same `absolute`, bit for bit: the
 *   bicubic resize of F.interpolate(mode='bicubic', align_corners=False) in that kernel's operation order (cubic_taps / cubic_row
 *   of daam_epilogue.h: Keys' weights with A = -0.75 in f32, the x pass on four rows and then the y pass, every product and sum
 *   rounded on its own, contraction off; a plane of the output's size is copied), then, unless `absolute`,
 *   (v - lo) / (hi - lo + 1e-8f) with lo / hi the exact minimum / maximum of the resized values (heatmap.py:77-93).
 *
 *   boxes      [n_words][n_thr][4] int32  x0 y0 x1 y1, inclusive: the bounding box of {p : v_j(p) > f32(thresholds[t])}; an
 *              empty set gives (out_w, out_h, -1, -1).                                        NULL iff n_words * n_thr == 0
 *   peaks      [n_words][2] int32  x, y of the pixel with the largest raw resized value; on a tie the lowest row-major index.
 *              Values are compared in the order of the integer encoding the minimum / maximum use (enc_ordered of
 *              daam_epilogue.h), which is the order of the floats but for -0 sorting below +0.  NULL iff n_words == 0
 *   peak_values[n_words][3] fp32  the raw resized value at the peak, then the exact minimum and maximum of the resized values (the
 *              first and the third are the same number).                                      NULL iff n_words == 0
 *   truth_boxes[n_truth][4] int32  the box of the set bytes of truth mask g, the same empty sentinel.   NULL iff n_truth == 0
 *   hits       [n_words][n_truth] uint8  truth_g[peaks[j]] != 0 as 0 / 1.                     NULL iff n_words * n_truth == 0
 * All outputs are overwritten in full by the call.  Every result is an integer or an exact f32 minimum / maximum joined by integer
 * atomics, so nothing depends on the grid, on the order in which workgroups run, or on the other words, thresholds or truth masks
 * of the call.  Every truth byte is fetched once (and n_words * n_truth of them once more, at the peaks).
 *
 * workspace: at least daam_localize_workspace(...) bytes of the same arguments, 8-byte aligned, the caller's between calls; it
 * holds the row and column maxima, the minima and the peak keys and is the only memory written besides the five outputs.
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): those above; workspace not NULL, large enough and
 * 8-byte aligned; thresholds finite. */
DAAM_API int    daam_localize(const float* word_maps, int n_words, int h, int w, int out_h, int out_w, int absolute,
                              const float* thresholds, int n_thr, const uint8_t* truth, int n_truth,
                              int32_t* boxes, int32_t* peaks, float* peak_values, int32_t* truth_boxes, uint8_t* hits,
                              void* workspace, size_t workspace_bytes, void* stream);
/* host only; 0 = out of range; monotone in each argument */
DAAM_API size_t daam_localize_workspace(int n_words, int n_truth, int n_thr, int out_h, int out_w);

DAAM_API int daam_locate_abi_version(void);            /* DAAM_LOCATE_ABI_VERSION */
DAAM_API const char* daam_locate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
