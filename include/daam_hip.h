/* daam_hip.h -- C ABI of libdaam_hip.so: the MI355X (gfx950) heat-map extraction path.
 *
 * This is the drop-in boundary for the ONE hot path of castorini/daam v0.2.0
 * (paths below are relative to the reference checkout):
 *
 *   tap       = what UNetCrossAttentionHooker.__call__ does between get_attention_scores and
 *               bmm (daam/trace.py:276-294): softmax(scale*Q K^T) -> keep the conditional
 *               half of the batch*heads dim -> [heads, tokens, h, w] -> per-(layer, head)
 *               running sum (RawHeatMapCollection.update, daam/heatmap.py:153-156).
 *   finalize  = DiffusionHeatMapHooker.compute_global_heat_map (daam/trace.py:103-130):
 *               key filter -> bicubic resize to x*x -> clamp(min=0) -> mean over keys
 *               (-> token crop is a view; optional per-pixel normalisation = epilogue).
 *   word maps = GlobalHeatMap.compute_word_heat_map + WordHeatMap.expand_as
 *               (daam/heatmap.py:121-123, 77-93)  [SURVEY.md section 8f row f1].
 *   overlap   = evaluate.compute_iou / compute_ioa (daam/evaluate.py:14-35)  [row f4].
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch types.
 *   - every `const void*` / `void*` data pointer is a DEVICE pointer owned by the caller
 *     unless the parameter is documented as "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every call only
 *     ENQUEUES work on that stream and returns; nothing synchronises the host except
 *     daam_ctx_destroy and the (rare) wrap-around of the internal upload ring.
 *   - return value: 0 = ok; > 0 = a hipError_t from the HIP runtime; < 0 = DAAM_E_* below.
 *     daam_last_error() gives the message of the last failure on the calling thread.
 *   - not thread-safe per context (the reference is not re-entrant either: it serialises
 *     generation with a lock, daam/run/demo.py:69,88).
 *   - a context belongs to the HIP device that was current at daam_ctx_create; its entry points switch to that
 *     device for the duration of the call when another one is current.
 */
#ifndef DAAM_HIP_H
#define DAAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAAM_ABI_VERSION 6

/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#define DAAM_API __attribute__((visibility("default")))

/* element types of activations (q, k, probs) and of the running sums */
#define DAAM_F16 0
#define DAAM_F32 1
#define DAAM_BF16 2         /* bfloat16 pipelines: bf16 logits / probabilities / sums (MFMA taps for every head_dim that is a multiple of 8, <= 256) */

/* DAAM_E_* */
#define DAAM_E_INVALID   (-1)   /* bad argument / shape / dtype */
#define DAAM_E_STATE     (-2)   /* call not valid in the current state (e.g. layer not configured) */
#define DAAM_E_NOMAPS    (-3)   /* finalize selected zero keys (reference: RuntimeError, trace.py:118-124) */
#define DAAM_E_UNSUPPORTED (-4)

typedef struct DaamCtx DaamCtx;

/* How one cross-attention call lays out its projected query / key.
 * Logical q is [batch, heads, hw, head_dim], k is [batch, heads, tokens, head_dim]; head_dim is
 * contiguous (stride 1), the other strides are given in ELEMENTS so that both the
 * head_to_batch_dim layout [B*H, S, d] (trace.py:272-273) and the raw to_q/to_k output
 * [B, S, H*d] (trace.py:262,269) can be tapped without a copy.
 * The reference keeps batch*heads indices [BH/2, BH) (trace.py:240): with classifier-free
 * guidance (batch 2) that is the conditional prompt, all heads. */
typedef struct DaamQKDesc {
    int32_t in_dtype;        /* DAAM_F16 | DAAM_F32 | DAAM_BF16: dtype of q and k (the pipeline dtype) */
    int32_t batch;           /* B */
    int32_t heads;           /* H */
    int32_t hw;              /* query positions = h*w (trace.py:233), pixel (p / w, p % w) */
    int32_t tokens;          /* key positions; only ctx->tokens (77) is tapped (trace.py:289) */
    int32_t head_dim;        /* d */
    int32_t round_logits;    /* 1: round scale*q.k to in_dtype before softmax (baddbmm output
                                dtype in diffusers get_attention_scores); 0: upcast_attention */
    float   scale;           /* attn.scale = head_dim ** -0.5 */
    int64_t q_stride_b, q_stride_h, q_stride_p;
    int64_t k_stride_b, k_stride_h, k_stride_t;
} DaamQKDesc;

/* ---- context ---------------------------------------------------------------------------
 * One context per trace object per device (reference: one RawHeatMapCollection per
 * DiffusionHeatMapHooker, trace.py:31).  tokens = context_size (77, trace.py:194);
 * out_side = int(sqrt(latent_hw)) (64, or 96 for 768-px SD-2.x; trace.py:32-33,109);
 * acc_dtype = dtype of the running sums: DAAM_F16 / DAAM_BF16 reproduce the reference's fp16 / bf16
 * sums on an fp16 / bf16 pipeline bit-for-bit in the add (heatmap.py:156), DAAM_F32 is the accuracy
 * mode.  Activations must have the dtype of the sums, or the sums must be DAAM_F32. */
DAAM_API int daam_ctx_create(int max_layers, int tokens, int out_side, int acc_dtype, DaamCtx** out);
DAAM_API int daam_ctx_destroy(DaamCtx* ctx);
/* Non-square generations (same ABI version: additive).  The reference fixes a square latent (latent_hw, trace.py:32-33) and takes
 * x = int(sqrt(latent_hw)) as the map side (trace.py:109); a generation of height x width pixels has out_h x out_w map cells
 * instead (1 <= out_h, out_w <= 128), and the bicubic of trace.py:116 resizes each [h, w] plane to it with one tap table per axis.
 * daam_ctx_create(.., s, ..) is daam_ctx_create_rect(.., s, s, ..).  On a context with
 * out_h != out_w -- or with a layer of unequal sides -- daam_finalize and daam_finalize_groups run finalize_rect_kernel
 * (daam_finalize_rect.hip: separable bicubic with one tap table per axis, f32 arithmetic on any finite planes, the
 * err_t <= 2^-19 * rowmax_t class below; DAAM_E_UNSUPPORTED when a selection's planes need more than 160 KB of LDS), and
 * daam_ctx_set_time_bins and daam_finalize_prepare are DAAM_E_UNSUPPORTED (daam_finalize then clears its output itself), and so
 * is daam_finalize_bins whenever the call needs the window-range reduction: a group over more than one window, or two groups
 * over the same window and key set (also with a single window).  Groups of one window each with distinct key sets are served:
 * that is daam_finalize_groups. */
DAAM_API int daam_ctx_create_rect(int max_layers, int tokens, int out_h, int out_w, int acc_dtype, DaamCtx** out);

/* Declare layer `layer` (= position in UNetCrossAttentionLocator.locate order, trace.py:45,50):
 * `heads` = kept batch*heads entries (BH - BH/2), `side` = sqrt(hw), `factor` =
 * int(sqrt(latent_hw // hw)) (trace.py:285).  `acc` = caller-owned zero-initialised device
 * buffer [heads, tokens, side, side] of acc_dtype, or NULL to let the library allocate it. */
DAAM_API int daam_layer_configure(DaamCtx* ctx, int layer, int heads, int side, int factor, void* acc);
/* daam_layer_configure for a layer of h x w query positions: position p is pixel (p / w, p % w), row-major as the NCHW
 * activations are flattened (trace.py:233 reshapes to [heads, tokens, h, w] with h = w); `factor` = int(sqrt(out_h * out_w // (h * w)))
 * (trace.py:285 with latent_hw = out_h * out_w); `acc` is [heads, tokens, h, w].  The taps read only h * w (DaamQKDesc.hw).
 * daam_layer_configure(.., side, ..) is the h == w case.  DAAM_E_UNSUPPORTED for h != w on a time-binned context. */
DAAM_API int daam_layer_configure_rect(DaamCtx* ctx, int layer, int heads, int h, int w, int factor, void* acc);
DAAM_API int daam_layer_acc(DaamCtx* ctx, int layer, void** acc, size_t* bytes);
/* The caller is about to write into the layer's sums itself (RawHeatMapCollection.update called by hand,
 * heatmap.py:153-156): a zeroing still owed to the buffer since the last daam_reset is enqueued on `stream` first,
 * and the layer counts as holding sums (the next tap adds to them, the next daam_reset clears them). */
DAAM_API int daam_layer_touch(DaamCtx* ctx, int layer, void* stream);
/* Forget layer `layer`: the context drops its pointer to the sums (a library-owned buffer is freed) and never touches that
 * memory again -- not even for a zeroing still owed since daam_reset.  This is RawHeatMapCollection.clear()
 * (daam/heatmap.py:170-172) as seen from tensors the caller handed out before: the reference drops its dict and the old
 * tensors live on unchanged.  The layer must be configured again before its next tap.  DAAM_E_STATE with taps pending. */
DAAM_API int daam_layer_release(DaamCtx* ctx, int layer);

/* ---- time windows ------------------------------------------------------------------------
 * The reference adds every denoising step into one running sum per (layer, head) (heatmap.py:153-156) and leaves the time
 * axis of DiffusionHeatMapHooker (time_idx / time_callback, trace.py:38,61-62) unused.  daam_ctx_set_time_bins splits it:
 * window b covers the steps [first_step[b], first_step[b + 1]) (the last window is open-ended), 1 <= n_bins <= 64,
 * first_step[0] == 0, strictly increasing (HOST array).  Call it before any layer is configured.  A layer's sums then
 * become [n_bins][heads, tokens, side, side] (daam_layer_configure's caller-owned `acc` holds all windows, daam_layer_acc
 * reports all of them) and every tap -- daam_tap_qk, daam_tap_qk_enqueue*, daam_attend with tap != 0, daam_tap_probs -- adds
 * into the window of its step.  A tap's step is the number of taps of THAT layer since daam_reset (the t-th tapped call of a
 * layer is denoising step t in diffusers' loop, with or without guidance; calls the reference's gate does not tap,
 * trace.py:289, never reach the library).  The deferred launch is unchanged: one table entry per (window, layer) chain.
 * On a binned context daam_layer_touch is DAAM_E_UNSUPPORTED, daam_finalize / daam_finalize_groups mean the whole generation
 * (windows [0, n_bins)) and daam_finalize_prepare is DAAM_E_UNSUPPORTED when n_bins > 1. */
DAAM_API int daam_ctx_set_time_bins(DaamCtx* ctx, int n_bins, const int32_t* first_step);
/* taps counted for `layer` since the last daam_reset (any context) */
DAAM_API int daam_tap_steps(DaamCtx* ctx, int layer, int* steps);

/* RawHeatMapCollection.clear (heatmap.py:170-172; called from check_inputs, trace.py:179):
 * zero every running sum and drop any un-flushed deferred taps. */
DAAM_API int daam_reset(DaamCtx* ctx, void* stream);

/* ---- tap -------------------------------------------------------------------------------
 * daam_tap_qk: one hooked cross-attention call, immediate: one kernel launch that
 * recomputes the conditional-half probabilities from q,k and adds them to the layer's sums.
 * daam_tap_qk_enqueue + daam_tap_flush: deferred form.  enqueue only records pointers (the
 * caller keeps q,k alive until the flush has been enqueued on `stream` and stream order
 * protects them); flush runs ALL recorded calls - every layer, every recorded step - as one
 * launch, adding the steps of a layer in the order they were recorded (so fp16 sums round
 * exactly like the reference's step-by-step adds) while reading and writing each running
 * sum once per flush instead of once per step.
 * daam_tap_probs: same accumulate from materialised probabilities [B*H, hw, tokens]
 * (the save_heads / load_heads path, trace.py:279-282, and any processor that already
 * holds attention_probs); bit-exact with the reference in the add.
 *
 * Logit domain (daam_tap_qk*, daam_attend; tests/test_gpu_softmax_domain.py).  The softmax is the reference's at any logit
 * magnitude the pipeline dtype holds: a pixel whose sum of exponentials leaves [2^-100, 2^100] is redone with its row maximum.
 * One exception, stated by its condition: a call with in_dtype = DAAM_F16, round_logits = 1 and a `scale` that is a positive
 * power of two (head_dim 64: 1/8, head_dim 16: 1/4 -- or any head_dim when the caller passes such a scale; it is a descriptor
 * field) on a context with the fast softmax (the default) keeps the UNSCALED q.k in fp16 and folds the scale into the exponent.
 * This holds for every kernel built on the 16x16 tile (tap_d64 / tap_wide / tap_walk / tap_pair / tap_chunk / tap_slab and the fp16
 * daam_attend).  Such a call requires |q.k| <= 65504 (|logit| <= 65504 * scale: 8188 at 1/8).  Beyond it the fp16 q.k is +-inf
 * and the pixel's 77 probabilities (and the pixel's daam_attend output row) are NaN where the reference, which rounds
 * q.k * scale, is finite; nothing checks this.  Outside the condition the limit does not exist: DAAM_STRICT_EXP=1 (read when the
 * context is created), a scale that is no power of two (head_dim 40 / 80 / 160 with head_dim^-1/2), round_logits = 0, bf16 and
 * f32 pipelines, and tap_mfma_kernel (DAAM_NO_D64=1) all scale before they round. */
DAAM_API int daam_tap_qk(DaamCtx* ctx, int layer, const void* q, const void* k, const DaamQKDesc* d, void* stream);
DAAM_API int daam_tap_qk_enqueue(DaamCtx* ctx, int layer, const void* q, const void* k, const DaamQKDesc* d);
/* the same as n daam_tap_qk_enqueue calls in order (all or nothing): lets a host runtime that
 * records calls cheaply hand them over in one crossing of the FFI.  HOST arrays. */
DAAM_API int daam_tap_qk_enqueue_many(DaamCtx* ctx, int n, const int32_t* layers, const void* const* q,
                             const void* const* k, const DaamQKDesc* const* descs);
DAAM_API int daam_tap_pending(DaamCtx* ctx, int* n_calls, int* max_steps);
DAAM_API int daam_tap_flush(DaamCtx* ctx, void* stream);
DAAM_API int daam_tap_probs(DaamCtx* ctx, int layer, const void* probs, int in_dtype, int batch_heads,
                   int hw, int tokens, void* stream);

/* ---- attend: the processor's attention with the tap fused in ---------------------------------
 * One cross-attention call of the reference's processor between the projections (daam/trace.py:262-270) and the
 * output projection (:300-302):  out = softmax(scale * Q K^T) V  for every (batch, head) -- get_attention_scores
 * (daam/trace.py:276) and torch.bmm(probs, value) + batch_to_head_dim (:296-297), with their rounding points: logits and
 * probabilities rounded to the pipeline dtype, the value product accumulated in f32 and rounded once -- and, when
 * `tap` != 0, the heat-map update of the same call (the per-head loop daam/trace.py:289-294, heatmap.py:153-156) from
 * the same probabilities, in the same kernel launch: nothing [B*H, hw, 77]-sized exists, Q is read once, no Q / K
 * has to stay alive after the call.  `tap` = 0 leaves the layer's sums alone (the caller records q, k for a deferred
 * daam_tap_qk_enqueue, or the call is not tapped: reference gate daam/trace.py:289).
 * v is [batch, tokens, heads * head_dim] like k; out is written as [batch, hw, heads * head_dim] in the given strides
 * (ELEMENTS; head_dim contiguous).  Supported: DAAM_F16 and DAAM_BF16 (bf16: round_logits = 1 only), head_dim a multiple of 8 up to 160 (SDXL / SD-2.x 64, SD-v1.5 40 /
 * 80 / 160), tokens 77, hw and strides multiples of 8, 16-byte aligned pointers -- daam_attend_supported() tells; otherwise DAAM_E_UNSUPPORTED and the
 * caller uses its framework's attention plus daam_tap_qk. */
typedef struct DaamAttendDesc {
    DaamQKDesc qk;
    int64_t v_stride_b, v_stride_h, v_stride_t;
    int64_t o_stride_b, o_stride_h, o_stride_p;
} DaamAttendDesc;
DAAM_API int daam_attend_supported(const DaamAttendDesc* d, const void* q, const void* k, const void* v, const void* out);
DAAM_API int daam_attend(DaamCtx* ctx, int layer, const void* q, const void* k, const void* v, void* out,
                         const DaamAttendDesc* d, int tap, void* stream);

/* ---- finalize ---------------------------------------------------------------------------
 * compute_global_heat_map (trace.py:103-126) over the keys selected by `key_mask`:
 * HOST array, one byte per (layer, head) in layer-major order over configured layers'
 * `heads` (offset of layer l = sum of heads of layers < l, see daam_key_offset), non-zero =
 * selected.  NULL selects every key.  Writes out[n_rows, out_side, out_side] fp32 =
 * mean over selected keys of clamp(bicubic(sum_plane), 0) for the token rows [0, n_rows).
 * `n_rows` (ABI v6): the reference crops the result to the prompt's n_tokens + 2 rows
 * (trace.py:127), so a caller that knows the prompt passes that count and the planes of the
 * other tokens are neither read nor written: the rows [0, n_rows) of `out` are overwritten, the
 * rows [n_rows, tokens) -- if `out` has them at all -- are left untouched.  n_rows <= 0 or
 * > tokens means all `tokens` rows.
 *
 * Value domain and accuracy (daam_finalize, daam_finalize_groups, daam_finalize_bins), per token row t against the exact result,
 * err_t = max over pixels of |out - exact|, rowmax_t = max over pixels of |exact| (tests/test_gpu_finalize_domain.py):
 *   - every class but 32 -> 64, and the 32 -> 64 class on the LDS kernel: f32 arithmetic on any finite planes,
 *     err_t <= 2^-19 * rowmax_t at any magnitude (measured: 2^-21.7).
 *   - the 32 -> 64 class on the matrix cores (the default for a 64 x 64 output: finalize_up32_pipe_kernel for all three dtypes of
 *     the sums, finalize_up32_mfma_kernel / finalize_up32_same_kernel for fp16 sums under DAAM_NO_PIPE_FINALIZE=1) passes f32 numbers
 *     -- the intermediate of the two bicubic passes, and the planes themselves when the sums are f32 -- to the fp16 matrix pipe as
 *     hi = fp16(v), lo = fp16(v - hi).  Two consequences.  DOMAIN: plane values must satisfy |v| <= 2^15 (beyond 65504 / 1.28, hi
 *     is inf and the map NaN; nothing checks this).  FLOOR: lo is an fp16 subnormal whenever |v| < 2^-3, so the split's error
 *     is an absolute 2^-25 rather than relative: err_t <= 2^-19 * rowmax_t + 2^-23 per map element (measured: 2^-20.2 and 2^-23.9),
 *     whatever the planes' magnitude.  Running sums of probabilities (<= steps x batch, start-of-text row of order steps) sit inside
 *     the domain and a content token whose row maximum is 1e-3 keeps 13 bits; planes fed through daam_tap_probs or summed far below
 *     2^-10 do not.  fp16 subnormal plane elements pass through the matrix pipe exactly (not flushed on gfx950).
 *   - the exact routes: DAAM_NO_PIPE_FINALIZE=1 for bf16 and f32 sums (LDS kernel), DAAM_NO_MFMA_FINALIZE=1 for fp16 sums (and
 *     every dtype); both are read when the context is created. */
DAAM_API int daam_key_offset(DaamCtx* ctx, int layer, int* offset, int* total);
DAAM_API int daam_finalize(DaamCtx* ctx, const uint8_t* key_mask, int n_rows, float* out, void* stream);
/* Optional, ABI v5 (`n_rows`: v6): announce the `key_mask` / `n_rows` / `out` / `stream` of the daam_finalize call that follows, BEFORE the deferred taps are
 * launched (between daam_tap_qk_enqueue* and daam_tap_flush), or any time before daam_finalize when nothing is pending.  The key /
 * pointer tables of the selection are kept on the device between calls (a generation's compute_global_heat_map, trace.py:103-126,
 * selects the same keys at the same addresses as the previous one) and `out` is cleared by the table-upload kernel of the tap
 * launch, so that daam_finalize itself is its class kernel(s) only.  `out` must stay allocated and untouched until that
 * daam_finalize; the announcement is one-shot and dropped by daam_reset, by a daam_finalize with other arguments (which then does
 * everything itself, as without this call) and by the next daam_tap_flush. */
DAAM_API int daam_finalize_prepare(DaamCtx* ctx, const uint8_t* key_mask, int n_rows, float* out, void* stream);

/* N global heat maps in one call (one prompt each, when a batch of N prompts was traced): key i (layer-major order, as key_mask)
 * belongs to group key_group[i] (HOST int32, one per key of daam_key_offset's `total`; -1 = not selected).  out[g] (device, fp32,
 * g * group_stride floats from `out`) = mean over the keys of group g of clamp(bicubic(plane), 0) for the token rows
 * [0, n_rows[g]) (HOST int32, the daam_finalize rule for <= 0 / > tokens); rows >= n_rows[g] of out[g] are left untouched.
 * 1 <= n_groups <= 64; a group with no keys: DAAM_E_NOMAPS.  n_groups == 1 is daam_finalize (and honours a
 * daam_finalize_prepare announcement of it).  Otherwise the call clears the groups' rows itself and launches each class kernel
 * ONCE for all groups (grouped forms: grid z = group); the device table cache of daam_finalize applies.  Exception: the round-2
 * MFMA x2 kernel behind DAAM_NO_PIPE_FINALIZE=1 serves a grouped call as one daam_finalize per group. */
DAAM_API int daam_finalize_groups(DaamCtx* ctx, const int32_t* key_group, int n_groups, const int32_t* n_rows,
                                  float* out, size_t group_stride, void* stream);

/* daam_finalize_groups with a window range per group: group g's map is computed from the sums of the windows
 * [bin_begin[g], bin_end[g]) added per key BEFORE the bicubic and the clamp (trace.py:118-124; the clamp is not linear) -- what the
 * reference computes from a generation that ran exactly those steps.  `key_group` indexes the key space of ONE window
 * (daam_key_offset); group g takes the keys whose entry equals group_set[g] (HOST int32 per group, >= 0), or g when group_set is
 * NULL -- so windows x prompts can share one prompt table (with group_set, keys of a set that no group takes are not selected).  bin_begin / bin_end / n_rows: HOST int32 per group,
 * 0 <= bin_begin[g] < bin_end[g] <= n_bins (1 on an un-binned context).  out / group_stride / rows as daam_finalize_groups.
 * Groups that each span one window run the grouped class kernels on that window's planes; otherwise one reduction launch adds the
 * windows' planes (rows [0, n_rows[g]) only) into f32 scratch planes first. */
DAAM_API int daam_finalize_bins(DaamCtx* ctx, const int32_t* key_group, int n_groups, const int32_t* group_set,
                                const int32_t* bin_begin, const int32_t* bin_end, const int32_t* n_rows, float* out,
                                size_t group_stride, void* stream);

/* trace.py:129-130: maps[:n_rows] / (maps[1:n_rows-1].sum(0) + 1e-6), in place on the first
 * n_rows planes of `maps` [*, side, side] fp32. */
DAAM_API int daam_epilogue_normalize(float* maps, int n_rows, int side, void* stream);
/* the same on planes of h x w (trace.py:129-130 does not look at the shape); the square call is h == w == side */
DAAM_API int daam_epilogue_normalize_rect(float* maps, int n_rows, int h, int w, void* stream);

/* ---- word maps (next row f1) -------------------------------------------------------------
 * heatmap.py:121-123 + 77-93: mean of the planes `idx[0..n_idx)` (HOST int array) of
 * maps[*, side, side] -> bicubic to out_h x out_w -> (absolute ? id : min-max normalise with
 * eps 1e-8) -> (threshold != 0 ? (x > threshold) : x).  word_map[side*side] (required) receives
 * the un-expanded mean plane; `out` [out_h, out_w] fp32 (NULL: only the mean plane is computed);
 * `workspace` >= 2 floats of device scratch for the min/max. */
DAAM_API int daam_word_heat_map(const float* maps, int side, const int32_t* idx, int n_idx, float* word_map,
                       float* out, int out_h, int out_w, int absolute, float threshold,
                       float* workspace, void* stream);
/* the same from maps[*, h, w]: word_map is [h * w], the bicubic reads a rectangular source (heatmap.py:77-93 generalised: the
 * reference's F.interpolate takes any source shape); the square call is h == w == side */
DAAM_API int daam_word_heat_map_rect(const float* maps, int h, int w, const int32_t* idx, int n_idx, float* word_map,
                       float* out, int out_h, int out_w, int absolute, float threshold,
                       float* workspace, void* stream);

/* Masks and a label map for many words in three launches (same ABI version: additive).  `idx` / `idx_begin[n_words + 1]` are HOST
 * arrays: word j owns the planes idx[idx_begin[j] .. idx_begin[j + 1]) of maps[rows, h, w] (h, w <= 128); idx_begin[0] == 0,
 * 1 <= n_words <= 32, every word non-empty, at most 255 indices in total, every index in [0, rows), words may share planes;
 * out_h, out_w >= 1, `threshold` finite -- anything else is DAAM_E_INVALID before any launch.
 *   word_maps [n_words, h, w] fp32 (required): word_maps[j] is bit for bit the word_map of daam_word_heat_map[_rect] on word j.
 *   v_j(p) = what daam_word_heat_map[_rect] writes to `out` for word j with the same `absolute` and threshold 0.
 *   masks  [n_words, out_h, out_w] uint8 or NULL: masks[j][p] = v_j(p) > threshold.
 *   labels [out_h, out_w] uint8 or NULL: the smallest j with v_j(p) = max_j v_j(p) when that maximum is > threshold, else 255.
 * `workspace` >= 2 * n_words floats of device scratch (the min / max pairs, started anew by every call).  Planes are assumed
 * finite.  No fp32 plane of out_h x out_w is written anywhere. */
DAAM_API int daam_word_masks(const float* maps, int rows, int h, int w, const int32_t* idx, const int32_t* idx_begin, int n_words,
                       float* word_maps, int out_h, int out_w, int absolute, float threshold, uint8_t* masks, uint8_t* labels,
                       float* workspace, void* stream);

/* ---- evaluation (next row f4) --------------------------------------------------------------
 * evaluate.compute_iou / compute_ioa (daam/evaluate.py:14-35) and WordHeatMap.compute_ioa (daam/heatmap.py:95-96) for a
 * batch of n pairs: a [n, a_h, a_w] (prediction) and b [n, b_h, b_w] (truth), fp32.  When a_h != b_h -- the reference tests
 * shape[0] only -- a is resized to (b_h, b_w) with the bicubic of F.interpolate and binarised (a < 1 -> 0, else 1); then
 * sums[i] = { sum(a * b), sum(a), sum(b) }  (sums [n, 3] fp32, overwritten).  The caller forms
 * IoU = s0 / (s1 + s2 - s0 + 1e-8) and IoA = s0 / (s1 + 1e-8) in fp32. */
DAAM_API int daam_mask_overlap(const float* a, int a_h, int a_w, const float* b, int b_h, int b_w, int n_pairs, float* sums,
                               void* stream);

/* The overlap matrix of two stacks of u8 masks in one pass (same ABI version: additive): what compute_iou / compute_ioa
 * (daam/evaluate.py:14-35) need for every prediction against every truth mask, and WordHeatMap.compute_ioa (daam/heatmap.py:95-96)
 * for every pair of words of one prompt, e.g. on the masks daam_word_masks leaves on the device.
 * a: [n_a, h, w] uint8, b: [n_b, h, w] uint8 (contiguous planes; a byte != 0 is "set"); b == NULL means b = a, n_b = n_a.
 * inter[i * n_b + j] = #{p : a_i[p] != 0 && b_j[p] != 0}, area_a[i] = #{p : a_i[p] != 0}, area_b[j] likewise (uint32, device).
 * 1 <= n_a, n_b <= 32, 1 <= h, w, h * w < 2^31.  The call overwrites all three outputs itself; area_b may be NULL when b is.
 * Base pointers need no alignment beyond one byte (a plane of an odd-sized stack starts anywhere).  Counts are exact integers;
 * every mask byte is fetched once.  The caller forms IoU = inter / (area_a + area_b - inter + 1e-8), IoA = inter / (area_a + 1e-8). */
DAAM_API int daam_mask_overlap_matrix(const uint8_t* a, int n_a, const uint8_t* b, int n_b, int h, int w,
                                      uint32_t* inter, uint32_t* area_a, uint32_t* area_b, void* stream);

/* Region attribution (same ABI version: additive): how much of every token row's expanded heat map lies inside each of n_masks
 * regions, scores[g][m][t] = sum over the pixels p with masks[m][p] != 0 of E_t[p], where E_t is what daam_word_heat_map[_rect]
 * writes for the plane maps[g][t] with absolute = 1 and threshold 0 (daam/heatmap.py:77-93: the bicubic of F.interpolate to the
 * image size, no min-max, no threshold) -- the expansion generalised from one word plane to every row, and from a picture to its sum
 * under a mask.  A byte != 0 is "set", the convention of daam/evaluate.py (load_mask: alpha > 0; compute_iou / compute_ioa on 0 / 1
 * masks) and of daam_mask_overlap_matrix.  The expansion is linear, so the call pulls every mask back through the transpose of the
 * resize once -- footprint[m][i][j] = sum over set (y, x) of wy[y][i] wx[x][j], clamped taps folded onto the edge cell -- and a
 * score is a dot product of h * w terms.  No fp32 plane of H x W is written anywhere; every mask byte is fetched once.
 *   masks     [n_masks, H, W] uint8, contiguous planes, any byte alignment;  1 <= n_masks <= 32, H, W >= 1, H * W < 2^31
 *   maps      [n_sets, rows, h, w] fp32 or NULL (then scores must be NULL too: footprint and area only);  1 <= h, w <= 128,
 *             n_sets (<= 65535), rows >= 1
 *   footprint [n_masks, h, w] fp32 (required): at H == h && W == w the mask itself as 0.0 / 1.0
 *   scores    [n_sets, n_masks, rows] fp32;  area [n_masks] uint32: the exact count of set bytes
 *   workspace daam_region_scores_workspace(...) bytes of device scratch, 16-byte aligned (0: the sizes are outside the limits)
 * Anything outside the limits is DAAM_E_INVALID before any launch.  The call overwrites all its outputs itself.  No floating-point
 * atomics: the results for mask m are bit-identical from run to run and do not depend on the other masks of the call, nor on
 * where its plane starts in memory.  Sums are fp32 with short chains (DESIGN 3.13 counts the roundings).
 * daam_region_dots is the last step alone: further map sets against a footprint that a daam_region_scores call left. */
DAAM_API size_t daam_region_scores_workspace(int n_masks, int H, int W, int h, int w);
DAAM_API int daam_region_scores(const uint8_t* masks, int n_masks, int H, int W, const float* maps, int n_sets, int rows, int h, int w,
                                float* footprint, float* scores, uint32_t* area, void* workspace, void* stream);
DAAM_API int daam_region_dots(const float* footprint, int n_masks, const float* maps, int n_sets, int rows, int h, int w,
                              float* scores, void* stream);

/* ---- misc -------------------------------------------------------------------------------- */
DAAM_API int daam_abi_version(void);
DAAM_API const char* daam_last_error(void);
/* per-kernel launch statistics of the last tap / finalize launch (for bench.py):
 * grid size and dynamic LDS bytes; 0 if nothing launched yet. */
DAAM_API int daam_last_launch(DaamCtx* ctx, int which /*0 tap,1 finalize*/, int* grid, int* block, int* lds_bytes);
/* launch structure of the last daam_tap_flush that launched something: kernels launched (one per kernel kind: SD-v1.5 has
 * head_dim 40 / 80 / 160 = three), how many of them went to auxiliary streams beside the caller's, the longest per-layer
 * step chain of the launch; `n_flushes` counts such flushes since daam_ctx_create (tests and bench.py assert the launch
 * structure a configuration is supposed to have: launches per generation, side-by-side kernels). Any pointer may be NULL. */
DAAM_API int daam_last_flush(DaamCtx* ctx, int* n_kernels, int* n_side_streams, int* max_steps, long long* n_flushes);
/* ABI v6: the names of the kernel(s) the last daam_tap_flush / daam_tap_qk (`which` 0) or daam_finalize (`which` 1) really launched,
 * '+'-separated in launch order (e.g. "tap_slab_kernel", "finalize_up32_pipe_kernel<f16>+finalize_up_kernel<16>"), copied into the HOST
 * buffer `names` (NUL-terminated, truncated to `capacity`); "" if nothing launched yet.  A report names what ran, not what the
 * environment asked for. */
DAAM_API int daam_last_kernels(DaamCtx* ctx, int which /*0 tap,1 finalize*/, char* names, int capacity);
/* kernel timing for bench.py: when enabled, every tap / finalize call brackets ITS KERNEL LAUNCHES (not
 * the table upload before them) with HIP events on the call's stream; daam_profile_last_ms waits for the
 * last pair and returns the elapsed milliseconds (the only other call that synchronises the host). */
DAAM_API int daam_profile_enable(DaamCtx* ctx, int on);
DAAM_API int daam_profile_last_ms(DaamCtx* ctx, int which /*0 tap,1 finalize*/, float* ms);
/* daam_profile_enable(ctx, 2): every launch of a kind gets its own event pair (a ring of 256), so that a whole timed region can be
 * measured without a host synchronisation inside it; daam_profile_history then returns the durations (ms, oldest first) of the last
 * min(launches since the enable, 256, capacity) launches of `which`. */
DAAM_API int daam_profile_history(DaamCtx* ctx, int which /*0 tap,1 finalize*/, float* ms, int capacity, int* n);
/* Shader-clock monitor for issue-rate rooflines: one wave on an internal stream takes `n_samples` (<= 4096) samples, `period_us`
 * apart, of the shader-cycle counter (s_memtime) and the constant 100 MHz reference counter (s_memrealtime) while the caller
 * runs the kernels under test on its own stream; _read waits for the monitor and returns the clock of every sampling
 * interval in MHz (delta cycles / delta reference x 100) -- the sustained clock under THAT load, which no host-side
 * sampler resolves for a 2 ms kernel.  The kernels under test are not instrumented. */
DAAM_API int daam_clock_monitor_start(DaamCtx* ctx, int n_samples, int period_us);
DAAM_API int daam_clock_monitor_read(DaamCtx* ctx, float* mhz, int capacity, int* n_intervals);

#ifdef __cplusplus
}
#endif
#endif /* DAAM_HIP_H */
