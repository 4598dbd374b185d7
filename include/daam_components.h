/* daam_components.h -- C ABI of libdaam_components.so: connected components of byte masks on the MI355X (gfx950).
 *
 * Labels, areas, largest-blob boxes.  The evaluation chain (daam_word_masks, daam_mask_overlap_matrix, daam_region_scores,
 * daam_threshold_sweep, daam_localize) treats a thresholded mask as a bag of pixels; this call says which pixels belong together.
 * A component is a maximal set of set pixels joined by steps to the 4 (edge) or 8 (edge and corner) neighbours.  With
 *   root := the lowest row-major index y * w + x of a component,
 *   rank := the position of a component when the components of ONE mask are sorted by root, from 0 (the order in which
 *           scipy.ndimage.label numbers them: its label minus one),
 * every result is an integer that the masks alone fix: union-find whose unions always hang the larger root under the smaller ends
 * with every pixel pointing at its component's lowest index whatever the order in which workgroups run.
 *
 * Conventions: those of daam_locate.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only enqueue,
 * 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_components_last_error() gives the message of the last failure on the calling
 * thread.  The library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing
 * from the other libraries but this header's include of daam_hip.h (DAAM_E_*).
 */
#ifndef DAAM_COMPONENTS_H
#define DAAM_COMPONENTS_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_COMPONENTS_ABI_VERSION 1

/* masks [n_masks][h][w] uint8 (a byte != 0 is set; contiguous planes at any byte alignment), 0 <= n_masks <= 32 (a call with no
 *   masks launches nothing), h, w >= 1, h * w < 2^31.
 * connectivity: 4 or 8.   min_area >= 0.
 * keep: 0 none, 1 the components with area >= min_area, 2 the largest component only.
 * max_comp: rows of `comps` per mask, 0 .. 65536.
 *
 *   labels  [n_masks][h][w] int32 or NULL: the rank of the pixel's component, -1 on background.
 *   counts  [n_masks][2] int32: the components of the mask; those with area >= min_area.
 *   comps   [n_masks][max_comp][6] int32: row k is the component of rank k -- root, area, x0, y0, x1, y1 (inclusive) --; rows from
 *           counts[m][0] on hold the empty sentinel (-1, 0, w, h, -1, -1).  A mask with more components than max_comp leaves
 *           counts, labels, largest and kept exact: only the list is cut.                            NULL iff max_comp == 0
 *   largest [n_masks][6] int32, the same columns: the component with the greatest area, on a tie the one with the lowest root; an
 *           empty mask gives the empty sentinel.
 *   kept    [n_masks][h][w] uint8 0 / 1: the pixels of the components `keep` keeps (keep == 2 on an empty mask: all zero).
 *                                                                                                       NULL iff keep == 0
 * All outputs are overwritten in full by the call.  Nothing depends on the grid, on the order in which workgroups run, or on the
 * other masks of the call.  Every mask byte is fetched once.
 *
 * workspace: at least daam_mask_components_workspace(...) bytes of the same arguments, 8-byte aligned, the caller's between calls
 * (8 bytes per pixel -- a parent and an area -- and 4 per row segment of 256 columns); it is the only memory written besides the
 * outputs.
 *
 * Limits (host-checked, DAAM_E_INVALID with a message before any HIP call): those above; masks, counts and largest not NULL;
 * workspace not NULL, large enough and 8-byte aligned. */
DAAM_API int    daam_mask_components(const uint8_t* masks, int n_masks, int h, int w, int connectivity, int min_area, int keep,
                                     int max_comp, int32_t* labels, int32_t* counts, int32_t* comps, int32_t* largest, uint8_t* kept,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* host only; 0 = out of range; monotone in each argument */
DAAM_API size_t daam_mask_components_workspace(int n_masks, int h, int w, int max_comp);

DAAM_API int daam_components_abi_version(void);        /* DAAM_COMPONENTS_ABI_VERSION */
DAAM_API const char* daam_components_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
