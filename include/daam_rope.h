/* daam_rope.h -- C ABI of libdaam_rope.so: the rotary position embedding of a FLUX-class attention call, applied to up to four
 * tensors (Q, image K, text K ...) in ONE launch, on the MI355X (gfx950).
 *
 * A FLUX attention call rotates Q and K after their norms and before the softmax; a tap of that call has to read the rotated values,
 * rounded to the model's dtype exactly as the model's own attention sees them.  The contract:
 *
 *   x, out        fp16 or bf16 (DAAM_F16 / DAAM_BF16), seen as [batch][rows][heads][d]; d is contiguous, the batch, row and head strides
 *                 are given in ELEMENTS, so that what the projections produce, [batch, rows, heads d], a row range of it and a packed
 *                 [batch, heads, rows, d] are all read and written without a copy
 *   cos, sin      f32 [rows][d], rows table_stride floats apart, ALREADY offset to the first row of the job (a job over the image rows
 *                 of a [text; image] table passes table + T * table_stride); a row is shared by every batch entry and head
 *   arithmetic    diffusers' apply_rotary_emb(x, (cos, sin), use_real=True, use_real_unbind_dim=-1), interleaved pairs: for c = 2 j
 *
 *                     out[c]     = rn( fadd( fmul(f32(x[c]),     cos[c]),     fmul(-f32(x[c + 1]), sin[c])     ) )
 *                     out[c + 1] = rn( fadd( fmul(f32(x[c + 1]), cos[c + 1]), fmul( f32(x[c]),     sin[c + 1]) ) )
 *
 *                 every fmul / fadd an IEEE f32 operation that is NOT contracted into an fma, rn round-to-nearest-even to the dtype of
 *                 x (an overflow to +-inf is the legal rounded result): the bits torch eager gives for
 *                 (x.float() * cos + x_rotated.float() * sin).to(x.dtype).  The result is exactly specified; there is no tolerance.
 *
 * Jobs are independent.  Within a job `out` must not overlap `x` (checked).  Two jobs whose outputs overlap, or a job that reads what
 * another job of the same call writes, are the caller's error: the result is UNDEFINED and nothing checks for it.  Elements of `out`
 * that lie between the rows and heads a job owns (strides larger than the data) are never written.
 *
 * No atomics, no workspace, no dependence on the grid: two runs give the same bits.  The kernel is in DESIGN 3.25.
 *
 * Conventions: those of daam_joint_tap.h -- extern "C", device pointers, `stream` a hipStream_t passed as void*, calls only enqueue,
 * 0 = ok / > 0 a hipError_t / < 0 DAAM_E_*; daam_rope_last_error() gives the message of the last failure on the calling thread.  The
 * library holds no context and no state between calls, and works on the HIP device that is current.  It needs nothing from the other
 * libraries but this header's include of daam_hip.h (DAAM_E_*, DAAM_F16, DAAM_BF16).
 */
#ifndef DAAM_ROPE_H
#define DAAM_ROPE_H

#include "daam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_ROPE_ABI_VERSION 1
#define DAAM_ROPE_MAX_JOBS 4
#define DAAM_ROPE_MAX_ROWS 16896             /* 16384 image cells + 512 text rows */
#define DAAM_ROPE_MAX_SLICES 4096            /* batch * heads */

typedef struct {
    const void* x;                           /* 16-byte aligned, read-only */
    void* out;                               /* 16-byte aligned */
    const float* cos;                        /* 16-byte aligned, already at this job's first row */
    const float* sin;
    int batch, heads, rows;                  /* each >= 1, batch * heads <= 4096, rows <= 16896 */
    int64_t x_stride_b, x_stride_r, x_stride_h;          /* elements: >= 0, multiples of 8; row and head strides >= d */
    int64_t out_stride_b, out_stride_r, out_stride_h;
    int64_t table_stride;                    /* floats between two rows of cos and of sin: >= d, a multiple of 4 */
} daam_rope_job;

/* jobs: HOST memory, n_jobs in 1..DAAM_ROPE_MAX_JOBS of them, copied into the launch; dtype DAAM_F16 or DAAM_BF16 for every x and
 * out; d 64 or 128.  One launch.  Every limit above is checked on the host (DAAM_E_INVALID with a message) before any HIP call. */
DAAM_API int daam_rope_apply(const daam_rope_job* jobs, int n_jobs, int dtype, int d, void* stream);

DAAM_API int daam_rope_abi_version(void);                     /* DAAM_ROPE_ABI_VERSION */
DAAM_API const char* daam_rope_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
