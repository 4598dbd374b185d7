// The epilogue on finished global maps, kernels and entry points:
//   * normalize_kernel                : daam/trace.py:129-130                         (daam_epilogue_normalize[_rect])
//   * word_mean / expand / post kernel: daam/heatmap.py:121-123, 77-93                (daam_word_heat_map[_rect])
//   * mask_overlap_kernel             : daam/evaluate.py:14-35 for a batch of pairs   (daam_mask_overlap)
// The batched forms live in daam_word_masks.hip, daam_mask_matrix.hip and daam_region_scores.hip; the text they share with this file is
// daam_epilogue.h.
#include "daam_ctx.h"
#include "daam_epilogue.h"

namespace daam {

// trace.py:129-130  maps[:n] / (maps[1:n-1].sum(0) + 1e-6)
__global__ __launch_bounds__(256) void normalize_kernel(float* maps, int n_rows, int plane)
{
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= plane) return;
    float s = 0.f;
    for (int t = 1; t < n_rows - 1; ++t) s += maps[(size_t)t * plane + px];
    s += 1e-6f;
    for (int t = 0; t < n_rows; ++t) maps[(size_t)t * plane + px] /= s;
}

// ---------------------------------------------------------------------------------------
// Word heat map (heatmap.py:121-123) and expand_as (heatmap.py:77-93).
// ---------------------------------------------------------------------------------------
struct WordIdx { int32_t n; int32_t idx[kMaxTokens]; };

__global__ __launch_bounds__(256) void word_mean_kernel(const float* maps, int plane, WordIdx w, float* word_map,
                                                        float* minmax)
{
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the start of the atomicMin / atomicMax pair of the expand kernels
        reinterpret_cast<int*>(minmax)[0] = kEncPosInf;
        reinterpret_cast<int*>(minmax)[1] = kEncNegInf;
    }
    if (px >= plane) return;
    float s = 0.f;
    for (int i = 0; i < w.n; ++i) s += maps[(size_t)w.idx[i] * plane + px];
    word_map[px] = s / (float)w.n;
}

// The two expand kernels are one body (daam_word_expand_body.inc) included under two spellings of the source size: as a force-inlined
// function called by both, by value or by reference, either kernel comes out as other machine code.
__global__ __launch_bounds__(256) void word_expand_kernel(const float* word_map, int side, float* out, int out_h,
                                                          int out_w, float* minmax)
{
#define SRC_H side
#define SRC_W side
#include "daam_word_expand_body.inc"
#undef SRC_H
#undef SRC_W
}

// a source plane of unequal sides (daam_word_heat_map_rect)
__global__ __launch_bounds__(256) void word_expand_rect_kernel(const float* word_map, int src_h, int src_w, float* out, int out_h,
                                                               int out_w, float* minmax)
{
#define SRC_H src_h
#define SRC_W src_w
#include "daam_word_expand_body.inc"
#undef SRC_H
#undef SRC_W
}

__global__ __launch_bounds__(256) void word_post_kernel(float* out, int n, const float* minmax, int absolute,
                                                        float threshold)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = out[i];
    if (!absolute) {
        const float lo = dec_ordered(reinterpret_cast<const int*>(minmax)[0]);
        const float hi = dec_ordered(reinterpret_cast<const int*>(minmax)[1]);
        v = (v - lo) / (hi - lo + 1e-8f);
    }
    if (threshold != 0.f) v = v > threshold ? 1.f : 0.f;      // `if threshold:` (heatmap.py:85)
    store_for_host(out + i, v);
}

// ---------------------------------------------------------------------------------------
// evaluate.compute_iou / compute_ioa (reference daam/evaluate.py:14-35) for a batch of (prediction, truth) pairs.
// One thread per pixel of the truth mask b; when the shapes differ (the reference tests shape[0] only) the prediction a is
// resized with the bicubic of F.interpolate (align_corners=False, A = -0.75, border-clamped taps; x on the four source rows,
// then y) and binarised (a < 1 -> 0, else 1); sums[pair] += {a*b, a, b}, one f32 atomic per wave and quantity -- exact for
// binary masks (integer sums below 2^24), order-dependent in the last bits for soft ones.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_overlap_kernel(const float* a, int a_h, int a_w, const float* b, int b_h, int b_w,
                                                           int resize, float* sums)
{
#pragma clang fp contract(off)
    const int pair = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* ap = a + (size_t)pair * a_h * a_w;
    float va = 0.f, vb = 0.f;
    if (i < b_h * b_w) {
        vb = b[(size_t)pair * b_h * b_w + i];
        if (!resize) {
            va = ap[i];
        } else {
            const int oy = i / b_w, ox = i - oy * b_w;
            float wy[4], wx[4];
            int iy[4], ix[4];
            {
                const int first = cubic_taps((float)a_h / (float)b_h, oy, wy);
                for (int t = 0; t < 4; ++t) iy[t] = min(max(first + t, 0), a_h - 1);
            }
            {
                const int first = cubic_taps((float)a_w / (float)b_w, ox, wx);
                for (int t = 0; t < 4; ++t) ix[t] = min(max(first + t, 0), a_w - 1);
            }
            float rows[4];
            for (int t = 0; t < 4; ++t) rows[t] = cubic_row(ap + (size_t)iy[t] * a_w, ix, wx);
            const float v = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
            va = v < 1.0f ? 0.0f : (v >= 1.0f ? 1.0f : v);    // a[a < 1] = 0; a[a >= 1] = 1  (evaluate.py:17-18): a NaN stays a NaN
        }
    }
    float inter = va * vb, sa = va, sb = vb;
    for (int off = 32; off > 0; off >>= 1) {
        inter += __shfl_xor(inter, off, 64);
        sa += __shfl_xor(sa, off, 64);
        sb += __shfl_xor(sb, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(sums + 3 * pair + 0, inter);
        atomicAdd(sums + 3 * pair + 1, sa);
        atomicAdd(sums + 3 * pair + 2, sb);
    }
}

}  // namespace daam

int daam_epilogue_normalize(float* maps, int n_rows, int side, void* stream)
{
    return daam_epilogue_normalize_rect(maps, n_rows, side, side, stream);
}

int daam_epilogue_normalize_rect(float* maps, int n_rows, int h, int w, void* stream)
{
    if (!maps || n_rows <= 0 || h <= 0 || w <= 0) return fail(DAAM_E_INVALID, "bad argument");
    const int plane = h * w;
    hipLaunchKernelGGL(normalize_kernel, dim3((plane + 255) / 256), dim3(256), 0, (hipStream_t)stream, maps, n_rows, plane);
    return launched("normalize");
}

int daam_word_heat_map(const float* maps, int side, const int32_t* idx, int n_idx, float* word_map, float* out,
                       int out_h, int out_w, int absolute, float threshold, float* workspace, void* stream)
{
    return daam_word_heat_map_rect(maps, side, side, idx, n_idx, word_map, out, out_h, out_w, absolute, threshold, workspace, stream);
}

int daam_word_heat_map_rect(const float* maps, int h, int w, const int32_t* idx, int n_idx, float* word_map, float* out,
                            int out_h, int out_w, int absolute, float threshold, float* workspace, void* stream)
{
    if (!maps || !idx || !word_map || !workspace) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_idx <= 0 || n_idx > kMaxTokens) return fail(DAAM_E_INVALID, "n_idx %d not in 1..%d", n_idx, kMaxTokens);
    if (h <= 0 || w <= 0 || (out && (out_h <= 0 || out_w <= 0))) return fail(DAAM_E_INVALID, "bad size");
    hipStream_t s = (hipStream_t)stream;
    WordIdx words;
    words.n = n_idx;
    for (int i = 0; i < n_idx; ++i) words.idx[i] = idx[i];
    const int plane = h * w;
    hipLaunchKernelGGL(word_mean_kernel, dim3((plane + 255) / 256), dim3(256), 0, s, maps, plane, words, word_map, workspace);
    if (out) {
        const int n = out_h * out_w;
        if (h == w)
            hipLaunchKernelGGL(word_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, s, word_map, h, out, out_h, out_w, workspace);
        else
            hipLaunchKernelGGL(word_expand_rect_kernel, dim3((n + 255) / 256), dim3(256), 0, s, word_map, h, w, out, out_h, out_w,
                               workspace);
        if (!absolute || threshold != 0.f)
            hipLaunchKernelGGL(word_post_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, n, workspace, absolute, threshold);
    }
    return launched("word map");
}

int daam_mask_overlap(const float* a, int a_h, int a_w, const float* b, int b_h, int b_w, int n_pairs, float* sums, void* stream)
{
    if (!a || !b || !sums) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_pairs <= 0 || n_pairs > 65535 || a_h <= 0 || a_w <= 0 || b_h <= 0 || b_w <= 0 || (long long)b_h * b_w > (1ll << 30))
        return fail(DAAM_E_INVALID, "bad shape: %d pairs, a %dx%d, b %dx%d", n_pairs, a_h, a_w, b_h, b_w);
    if (a_h == b_h && a_w != b_w)
        return fail(DAAM_E_INVALID, "same heights but widths %d / %d differ (the reference's a * b would not broadcast)", a_w, b_w);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * 3 * (size_t)n_pairs, s);
    if (e != hipSuccess) return launched("mask overlap", e);
    hipLaunchKernelGGL(mask_overlap_kernel, dim3((b_h * b_w + 255) / 256, n_pairs), dim3(256), 0, s, a, a_h, a_w, b, b_h, b_w,
                       a_h != b_h ? 1 : 0, sums);
    return launched("mask overlap");
}
