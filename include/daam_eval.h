/* daam_eval.h -- C ABI of libdaam_eval.so: segmentation evaluation on the MI355X (gfx950).
 *
 * Threshold sweep.  The masks of WordHeatMap.expand_as(image, threshold=tau) (reference daam/heatmap.py:77-93) and the IoU / IoA
 * computed from them (daam/evaluate.py:14-35) depend on one free parameter, tau, and an evaluation reports them as a curve over
 * tau.  For one (words, image size, truth masks) triple the expanded value of a pixel is the same at every tau; only a comparison
 * changes.  daam_threshold_sweep therefore bins every expanded value against the sorted thresholds once and counts it per truth
 * mask: the exact intersections and areas at ALL thresholds come from two passes at image resolution (a min / max pass, a binning
 * pass) whatever the number of thresholds, and nothing is written at image resolution.
 *
 * Conventions: those of daam_hip.h -- extern "C", device pointers unless documented otherwise, `stream` a hipStream_t passed as
 * void*, calls only enqueue, 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_eval_last_error() gives the message of the last
 * failure on the calling thread.  The library holds no context and no state between calls, and works on the HIP device that is
 * current.  It is separate from libdaam_hip.so and needs nothing from it but this header's include of daam_hip.h (DAAM_E_*).
 */
#ifndef DAAM_EVAL_H
#define DAAM_EVAL_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_EVAL_ABI_VERSION 1

/* thresholds: HOST array, finite, strictly increasing, 1 <= n_thr <= 64.
 * word_maps [n_words][h][w] fp32: the un-expanded mean planes, as daam_word_masks / daam_word_heat_map leave them;
 *   1 <= n_words <= 32, 1 <= h, w <= 128.  truth [n_truth][out_h][out_w] uint8 (byte != 0 is set; contiguous planes, any
 *   byte alignment), 0 <= n_truth <= 32 (0 with truth == NULL: predicted areas only).  out_h, out_w >= 1, out_h * out_w < 2^31.
 * v_j(p) := what daam_word_masks compares with its threshold for word j, pixel p, under the same `absolute` -- bit for bit.
 *   pred_area [n_words][n_thr]                 uint32 = #{p : v_j(p) > thresholds[t]}
 *   inter     [n_words][n_truth][n_thr]        uint32 = #{p : v_j(p) > thresholds[t] && truth_g[p] != 0}   (NULL iff n_truth == 0)
 *   truth_area[n_truth]                        uint32                                                      (NULL iff n_truth == 0)
 * All outputs are overwritten in full by the call.  No fp32 or u8 plane of out_h x out_w is written anywhere; every truth
 * byte is fetched once per call.
 *
 * Arithmetic.  v_j(p) is the bicubic resize of F.interpolate(mode='bicubic', align_corners=False) in the operation order of
 * daam_word_masks (Keys' weights with A = -0.75 in f32, the x pass on four rows and then the y pass, every product and sum
 * rounded on its own; a plane of the output's size is copied), then, unless `absolute`, (v - lo) / (hi - lo + 1e-8) in f32 with
 * lo / hi the exact minimum / maximum of word j's resized values (integer atomics on an order-preserving encoding: exact and
 * order-free).  A pixel's bin is #{t : v > f32(thresholds[t])} in 0 .. n_thr -- a NaN compares false everywhere and goes to bin
 * 0 -- and every output is a suffix sum of per-bin counts: pred_area[j][t] = the pixels of word j in bins t + 1 .. n_thr.
 * Everything counted is an integer; integer atomics join the workgroups, so no result depends on the grid, on the order in
 * which workgroups run, on the other words or truth masks of the call, or on how the call splits its words over the
 * workgroup's counters (n_words x (n_truth + 1) x (n_thr + 1) of them do not fit the LDS at the limits: a workgroup takes the
 * words in groups and keeps its pixels' taps and truth bits in registers between the groups).
 *
 * workspace: at least daam_threshold_sweep_workspace(...) bytes of the same arguments, 4-byte aligned, the caller's between
 * calls; it holds the min / max pairs and the per-bin counters and is the only memory written besides the three outputs.
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): those above; word_maps, thresholds, pred_area and
 * workspace not NULL; truth, inter and truth_area NULL exactly when n_truth == 0; thresholds finite and strictly increasing;
 * workspace_bytes large enough and workspace 4-byte aligned. */
DAAM_API int    daam_threshold_sweep(const float* word_maps, int n_words, int h, int w, int out_h, int out_w, int absolute,
                                     const float* thresholds, int n_thr, const uint8_t* truth, int n_truth,
                                     uint32_t* pred_area, uint32_t* inter, uint32_t* truth_area,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* host only; 0 = out of range; monotone in each argument */
DAAM_API size_t daam_threshold_sweep_workspace(int n_words, int n_truth, int n_thr, int out_h, int out_w);

DAAM_API int daam_eval_abi_version(void);              /* DAAM_EVAL_ABI_VERSION */
DAAM_API const char* daam_eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
