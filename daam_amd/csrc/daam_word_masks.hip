// daam_word_masks: the word maps of up to 32 words, their thresholded masks at image resolution and the label map ("which word
// owns this pixel") in three launches, whatever the number of words -- the batched form of daam_word_heat_map[_rect] (kernels:
// daam_epilogue.hip, daam_word_expand_body.inc), whose values it reproduces bit for bit without ever writing an f32 plane at image
// resolution:
//   * word_masks_mean_kernel   : every word's mean plane, and the +inf / -inf start of every word's min / max pair
//   * word_masks_minmax_kernel : min / max of every word's bicubic resize (stores nothing at image resolution; not launched when
//                                `absolute`)
//   * word_masks_out_kernel    : the same resize again -> normalise -> compare -> u8 masks, running arg-max -> u8 labels
// The two image-resolution kernels share expand_run(): a lane owns kRun consecutive x of one output row, computes its tap indices
// and weights once and reuses them over all words.  The arithmetic is that of daam_word_expand_body.inc and word_post_kernel
// (contraction off, same operand order) through the same helpers of daam_epilogue.h: cubic_taps, cubic_row, enc / dec_ordered.
// The source planes ([n_words, h, w] f32, <= 2 MB) are read through L1 / L2, not staged in LDS.
#include "daam_ctx.h"
#include "daam_epilogue.h"

#include <cmath>

namespace daam {

constexpr int kMaxWords = 32;
constexpr int kMaxWordIdx = 255;
#ifndef DAAM_WM_RUN
#define DAAM_WM_RUN 4                 // consecutive x per lane: a multiple of 4 (u8 results leave as dwords)
#endif
constexpr int kRun = DAAM_WM_RUN;
static_assert(kRun % 4 == 0 && kRun >= 4 && kRun <= 16, "a lane's run is whole dwords of u8");

// word j owns the planes idx[begin[j] .. begin[j + 1])
struct WordTable { int32_t n_words; int32_t begin[kMaxWords + 1]; int32_t idx[kMaxWordIdx]; };

// grid (ceil(plane / 256), n_words): block (b, j) writes 256 pixels of word j's mean plane (the sum order and the division of
// word_mean_kernel); block (0, j) starts word j's min / max pair
__global__ __launch_bounds__(256) void word_masks_mean_kernel(const float* maps, int plane, WordTable t, float* word_maps, float* minmax)
{
    const int j = blockIdx.y;
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the start of the atomicMin / atomicMax pair of word_masks_minmax_kernel
        reinterpret_cast<int*>(minmax)[2 * j] = kEncPosInf;
        reinterpret_cast<int*>(minmax)[2 * j + 1] = kEncNegInf;
    }
    if (px >= plane) return;
    const int b = t.begin[j], e = t.begin[j + 1];
    float s = 0.f;
    for (int i = b; i < e; ++i) s += maps[(size_t)t.idx[i] * plane + px];
    word_maps[(size_t)j * plane + px] = s / (float)(e - b);
}

// The run of one lane: output row oy, columns x0 .. x0 + kRun.  Rows / columns past the image are clamped to its last one, so every
// read is in bounds and the caller masks what it does with those values (`n_valid` of them count).
struct WordRun {
    int oy, x0, n_valid;
    bool identity;
    int iy[4], ix[kRun][4];
    float wy[4], wx[kRun][4];
};

__device__ __forceinline__ void wm_run_setup(WordRun& r, int src_h, int src_w, int out_h, int out_w)
{
#pragma clang fp contract(off)
    const int runs_per_row = (out_w + kRun - 1) / kRun;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int row = t / runs_per_row;
    r.x0 = (t - row * runs_per_row) * kRun;
    r.n_valid = row < out_h ? min(kRun, out_w - r.x0) : 0;
    r.oy = min(row, out_h - 1);
    r.identity = src_h == out_h && src_w == out_w;
    {
        const int first = cubic_taps((float)src_h / (float)out_h, r.oy, r.wy);
        for (int a = 0; a < 4; ++a) r.iy[a] = min(max(first + a, 0), src_h - 1);
    }
    const float sc = (float)src_w / (float)out_w;
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        const int first = cubic_taps(sc, min(r.x0 + k, out_w - 1), r.wx[k]);
        for (int a = 0; a < 4; ++a) r.ix[k][a] = min(max(first + a, 0), src_w - 1);
    }
}

// v[k] = what word_expand[_rect]_kernel writes at (oy, x0 + k) from the plane `word_map` [src_h][src_w]
__device__ __forceinline__ void expand_run(const WordRun& r, const float* word_map, int src_w, int out_w, float v[kRun])
{
#pragma clang fp contract(off)
    if (r.identity) {
#pragma unroll
        for (int k = 0; k < kRun; ++k) v[k] = word_map[r.oy * out_w + min(r.x0 + k, out_w - 1)];
        return;
    }
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        float rows[4];
        for (int a = 0; a < 4; ++a) rows[a] = cubic_row(word_map + r.iy[a] * src_w, r.ix[k], r.wx[k]);
        v[k] = rows[0] * r.wy[0] + rows[1] * r.wy[1] + rows[2] * r.wy[2] + rows[3] * r.wy[3];
    }
}

// one thread per run; per word one atomic min / max pair per wave
__global__ __launch_bounds__(256) void word_masks_minmax_kernel(const float* word_maps, int n_words, int src_h, int src_w, int out_h,
                                                                int out_w, float* minmax)
{
    WordRun r;
    wm_run_setup(r, src_h, src_w, out_h, out_w);
    const int plane = src_h * src_w;
#pragma unroll 1
    for (int j = 0; j < n_words; ++j) {
        float v[kRun];
        expand_run(r, word_maps + (size_t)j * plane, src_w, out_w, v);
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int k = 0; k < kRun; ++k)
            if (k < r.n_valid) {
                lo = fminf(lo, v[k]);
                hi = fmaxf(hi, v[k]);
            }
        for (int off = 32; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off, 64));
            hi = fmaxf(hi, __shfl_xor(hi, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(reinterpret_cast<int*>(minmax) + 2 * j, enc_ordered(lo));
            atomicMax(reinterpret_cast<int*>(minmax) + 2 * j + 1, enc_ordered(hi));
        }
    }
}

// kRun u8 results of one lane to dst[0 .. n): whole dwords when the run is complete and lands on a dword boundary (every run of an
// image whose width is a multiple of 4), element by element otherwise (row tails, rows of other widths)
__device__ __forceinline__ void wm_store_run(uint8_t* dst, const uint32_t packed[kRun / 4], int n)
{
    if (n == kRun && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < kRun / 4; ++q) reinterpret_cast<uint32_t*>(dst)[q] = packed[q];
    } else {
#pragma unroll
        for (int k = 0; k < kRun; ++k)
            if (k < n) dst[k] = (uint8_t)(packed[k >> 2] >> (8 * (k & 3)));
    }
}

// one thread per run: masks[j] = v_j > threshold, labels = the first j whose v_j is the largest when that is > threshold, else 255
__global__ __launch_bounds__(256) void word_masks_out_kernel(const float* word_maps, int n_words, int src_h, int src_w, int out_h,
                                                             int out_w, const float* minmax, int absolute, float threshold,
                                                             uint8_t* masks, uint8_t* labels)
{
#pragma clang fp contract(off)
    WordRun r;
    wm_run_setup(r, src_h, src_w, out_h, out_w);
    if (r.n_valid == 0) return;
    const int plane = src_h * src_w;
    const size_t n = (size_t)out_h * out_w;
    const size_t at = (size_t)r.oy * out_w + r.x0;
    float best[kRun];
    int best_j[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) { best[k] = -INFINITY; best_j[k] = 255; }
#pragma unroll 1
    for (int j = 0; j < n_words; ++j) {
        float v[kRun];
        expand_run(r, word_maps + (size_t)j * plane, src_w, out_w, v);
        if (!absolute) {
            const float lo = dec_ordered(reinterpret_cast<const int*>(minmax)[2 * j]);
            const float hi = dec_ordered(reinterpret_cast<const int*>(minmax)[2 * j + 1]);
#pragma unroll
            for (int k = 0; k < kRun; ++k) v[k] = (v[k] - lo) / (hi - lo + 1e-8f);
        }
        uint32_t packed[kRun / 4] = {};
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            packed[k >> 2] |= (v[k] > threshold ? 1u : 0u) << (8 * (k & 3));
            if (v[k] > best[k]) { best[k] = v[k]; best_j[k] = j; }
        }
        if (masks) wm_store_run(masks + (size_t)j * n + at, packed, r.n_valid);
    }
    if (labels) {
        uint32_t packed[kRun / 4] = {};
#pragma unroll
        for (int k = 0; k < kRun; ++k) packed[k >> 2] |= (uint32_t)(best[k] > threshold ? best_j[k] : 255) << (8 * (k & 3));
        wm_store_run(labels + at, packed, r.n_valid);
    }
}

}  // namespace daam

int daam_word_masks(const float* maps, int rows, int h, int w, const int32_t* idx, const int32_t* idx_begin, int n_words,
                    float* word_maps, int out_h, int out_w, int absolute, float threshold, uint8_t* masks, uint8_t* labels,
                    float* workspace, void* stream)
{
    if (!maps || !idx || !idx_begin || !word_maps || !workspace) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_words < 1 || n_words > kMaxWords) return fail(DAAM_E_INVALID, "n_words %d not in 1..%d", n_words, kMaxWords);
    if (rows < 1 || h < 1 || w < 1 || h > 128 || w > 128) return fail(DAAM_E_INVALID, "bad maps shape [%d, %d, %d] (h, w <= 128)", rows, h, w);
    if (out_h < 1 || out_w < 1 || (long long)out_h * out_w > (1ll << 30)) return fail(DAAM_E_INVALID, "bad output size %d x %d", out_h, out_w);
    if (!std::isfinite(threshold)) return fail(DAAM_E_INVALID, "threshold is not finite");
    if (idx_begin[0] != 0) return fail(DAAM_E_INVALID, "idx_begin[0] is %d, not 0", idx_begin[0]);
    WordTable t;
    t.n_words = n_words;
    t.begin[0] = 0;
    for (int j = 0; j < n_words; ++j) {
        if (idx_begin[j + 1] <= idx_begin[j]) return fail(DAAM_E_INVALID, "word %d is empty", j);
        if (idx_begin[j + 1] > kMaxWordIdx) return fail(DAAM_E_INVALID, "more than %d indices in total", kMaxWordIdx);
        t.begin[j + 1] = idx_begin[j + 1];
    }
    for (int j = n_words + 1; j <= kMaxWords; ++j) t.begin[j] = t.begin[n_words];
    const int total = idx_begin[n_words];
    for (int i = 0; i < kMaxWordIdx; ++i) {
        if (i < total && (idx[i] < 0 || idx[i] >= rows)) return fail(DAAM_E_INVALID, "index %d (position %d) not in [0, %d)", idx[i], i, rows);
        t.idx[i] = i < total ? idx[i] : 0;
    }
    hipStream_t s = (hipStream_t)stream;
    const int plane = h * w;
    hipLaunchKernelGGL(word_masks_mean_kernel, dim3((plane + 255) / 256, n_words), dim3(256), 0, s, maps, plane, t, word_maps, workspace);
    if (masks || labels) {
        const int runs = out_h * ((out_w + kRun - 1) / kRun);
        if (!absolute)
            hipLaunchKernelGGL(word_masks_minmax_kernel, dim3((runs + 255) / 256), dim3(256), 0, s, word_maps, n_words, h, w, out_h, out_w,
                               workspace);
        hipLaunchKernelGGL(word_masks_out_kernel, dim3((runs + 255) / 256), dim3(256), 0, s, word_maps, n_words, h, w, out_h, out_w,
                           workspace, absolute, threshold, masks, labels);
    }
    return launched("word masks");
}
