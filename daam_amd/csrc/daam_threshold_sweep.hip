// daam_threshold_sweep (include/daam_eval.h): the pixel counts behind IoU / IoA of up to 32 word masks against up to 32 truth masks at
// up to 64 thresholds, from two passes at image resolution whatever the number of thresholds.  The value compared is
// that of daam_word_masks.hip, restated here through the same helpers of daam_epilogue.h (cubic_taps, cubic_row, enc / dec_ordered;
// contraction off, the same operand order), so a count is bit for bit what word_masks_out_kernel's mask at that threshold holds:
//   * sweep_init_kernel     : the per-bin counters to zero, the +inf / -inf start of every word's min / max pair
//   * sweep_minmax_kernel   : min / max of every word's bicubic resize (not launched when `absolute`)
//   * sweep_count_kernel    : the same resize again -> normalise -> bin against the sorted thresholds -> counters [word][bin][column],
//                             column 0 = every pixel, column 1 + g = the pixels truth mask g sets
//   * sweep_finalize_kernel : suffix sums over the bins -> pred_area, inter, truth_area
// A lane owns kSwRun consecutive x of one output row (the run of daam_word_masks.hip), computes its taps once and fetches its truth
// bytes once; both stay in registers over all words.  Counting is per wave: for every distinct bin among the wave's 64 pixels one
// ballot gives the pixels in it, and lane c adds popcount(ballot & column c's pixels) to the workgroup's counter [word][bin][c] in
// LDS -- columns are consecutive addresses, and the pixels of a background that all fall into bin 0 cost one LDS add per column,
// not 64 on one address.  The counters of all words do not fit the LDS at the limits: the workgroup walks the words in groups,
// and flushes a group with one global integer atomic per non-zero counter.  Integers only: nothing depends on the grid or the order.
#include "daam_epilogue.h"
#include "../../include/daam_eval.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kSwMaxWords = 32;
constexpr int kSwMaxTruth = 32;
constexpr int kSwMaxThr = 64;
constexpr int kSwMaxSide = 128;
constexpr int kSwRun = 4;                       // consecutive x per lane: a lane's truth bytes are one dword
constexpr int kSwThreads = 256;
constexpr int kSwThrSlots = 2 * kSwMaxThr;      // the thresholds in LDS, padded with +inf: what the binary search may touch
constexpr int kSwHistCap = 12288;               // counters a workgroup holds at once (48 KB): three workgroups per CU at the limits
constexpr size_t kSwMinmaxBytes = 2 * kSwMaxWords * sizeof(int);

struct SweepArgs {
    const float* word_maps;
    const uint8_t* truth;
    int* minmax;                // [n_words][2], enc_ordered
    uint32_t* bins;             // [n_words][n_thr + 1][n_truth + 1]
    uint32_t* pred_area;
    uint32_t* inter;
    uint32_t* truth_area;
    int n_words, src_h, src_w, out_h, out_w, absolute, n_thr, n_truth;
    int group;                  // words whose counters a workgroup holds at once
    int top;                    // the largest power of two <= n_thr: the first step of the binary search
    float thr[kSwMaxThr];
};

__global__ __launch_bounds__(kSwThreads) void sweep_init_kernel(const SweepArgs a)
{
    const int t = blockIdx.x * kSwThreads + threadIdx.x;
    if (t < a.n_words * (a.n_thr + 1) * (a.n_truth + 1)) a.bins[t] = 0;
    if (t < a.n_words) {
        a.minmax[2 * t] = kEncPosInf;
        a.minmax[2 * t + 1] = kEncNegInf;
    }
}

// The run of one lane: output row oy, columns x0 .. x0 + kSwRun.  Rows / columns past the image are clamped to its last one, so
// every read is in bounds; `n_valid` of the run's values count.
struct SweepRun {
    int oy, x0, n_valid;
    bool identity;
    int iy[4], ix[kSwRun][4];
    float wy[4], wx[kSwRun][4];
};

__device__ __forceinline__ void sweep_run_setup(SweepRun& r, int src_h, int src_w, int out_h, int out_w)
{
#pragma clang fp contract(off)
    const int runs_per_row = (out_w + kSwRun - 1) / kSwRun;
    const unsigned t = blockIdx.x * kSwThreads + threadIdx.x;         // < 2^31 + 256: out_h * out_w < 2^31
    const unsigned row = t / (unsigned)runs_per_row;
    r.x0 = (int)(t - row * (unsigned)runs_per_row) * kSwRun;
    r.n_valid = row < (unsigned)out_h ? min(kSwRun, out_w - r.x0) : 0;
    r.oy = (int)min(row, (unsigned)out_h - 1u);
    r.identity = src_h == out_h && src_w == out_w;
    {
        const int first = cubic_taps((float)src_h / (float)out_h, r.oy, r.wy);
        for (int a = 0; a < 4; ++a) r.iy[a] = min(max(first + a, 0), src_h - 1);
    }
    const float sc = (float)src_w / (float)out_w;
#pragma unroll
    for (int k = 0; k < kSwRun; ++k) {
        const int first = cubic_taps(sc, min(r.x0 + k, out_w - 1), r.wx[k]);
        for (int a = 0; a < 4; ++a) r.ix[k][a] = min(max(first + a, 0), src_w - 1);
    }
}

// v[k] = what word_expand[_rect]_kernel writes at (oy, x0 + k) from the plane `word_map` [src_h][src_w]
__device__ __forceinline__ void sweep_expand_run(const SweepRun& r, const float* word_map, int src_w, int out_w, float v[kSwRun])
{
#pragma clang fp contract(off)
    if (r.identity) {
#pragma unroll
        for (int k = 0; k < kSwRun; ++k) v[k] = word_map[r.oy * out_w + min(r.x0 + k, out_w - 1)];
        return;
    }
#pragma unroll
    for (int k = 0; k < kSwRun; ++k) {
        float rows[4];
        for (int a = 0; a < 4; ++a) rows[a] = cubic_row(word_map + r.iy[a] * src_w, r.ix[k], r.wx[k]);
        v[k] = rows[0] * r.wy[0] + rows[1] * r.wy[1] + rows[2] * r.wy[2] + rows[3] * r.wy[3];
    }
}

// one thread per run; per word one atomic min / max pair per wave
__global__ __launch_bounds__(kSwThreads) void sweep_minmax_kernel(const SweepArgs a)
{
    SweepRun r;
    sweep_run_setup(r, a.src_h, a.src_w, a.out_h, a.out_w);
    const int plane = a.src_h * a.src_w;
#pragma unroll 1
    for (int j = 0; j < a.n_words; ++j) {
        float v[kSwRun];
        sweep_expand_run(r, a.word_maps + (size_t)j * plane, a.src_w, a.out_w, v);
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int k = 0; k < kSwRun; ++k)
            if (k < r.n_valid) {
                lo = fminf(lo, v[k]);
                hi = fmaxf(hi, v[k]);
            }
        for (int off = 32; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off, 64));
            hi = fmaxf(hi, __shfl_xor(hi, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(a.minmax + 2 * j, enc_ordered(lo));
            atomicMax(a.minmax + 2 * j + 1, enc_ordered(hi));
        }
    }
}

// one thread per run.  Dynamic LDS: the padded thresholds, then the counters [group][n_thr + 1][n_truth + 1]
__global__ __launch_bounds__(kSwThreads) void sweep_count_kernel(const SweepArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char sweep_smem[];
    float* const thr = reinterpret_cast<float*>(sweep_smem);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(thr + kSwThrSlots);
    const int tid = threadIdx.x, lane = tid & 63;
    const int cols = a.n_truth + 1, cells = (a.n_thr + 1) * cols;
    if (tid < kSwThrSlots) thr[tid] = tid < a.n_thr ? a.thr[tid] : INFINITY;

    SweepRun r;
    sweep_run_setup(r, a.src_h, a.src_w, a.out_h, a.out_w);

    // Column c's pixels among the wave's, per run position k, held by lane c: column 0 is every pixel of the image, column 1 + g
    // those whose byte of truth mask g is not zero.  A lane fetches its run's bytes of every truth mask here, once.
    unsigned long long valid[kSwRun], sel[kSwRun];
#pragma unroll
    for (int k = 0; k < kSwRun; ++k) {
        valid[k] = __ballot(k < r.n_valid);
        sel[k] = lane == 0 ? valid[k] : 0ull;
    }
    {
        const size_t n = (size_t)a.out_h * a.out_w;
        const size_t at = (size_t)r.oy * a.out_w + r.x0;
#pragma unroll 1
        for (int g = 0; g < a.n_truth; ++g) {
            const uint8_t* const p = a.truth + (size_t)g * n + at;
            uint32_t bytes = 0;
            if (r.n_valid == kSwRun && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                bytes = *reinterpret_cast<const uint32_t*>(p);
            } else {
#pragma unroll
                for (int k = 0; k < kSwRun; ++k)
                    if (k < r.n_valid) bytes |= (uint32_t)p[k] << (8 * k);
            }
#pragma unroll
            for (int k = 0; k < kSwRun; ++k) {
                const unsigned long long set = __ballot(((bytes >> (8 * k)) & 0xffu) != 0);
                if (lane == g + 1) sel[k] = set & valid[k];
            }
        }
    }

    const int plane = a.src_h * a.src_w;
    for (int j0 = 0; j0 < a.n_words; j0 += a.group) {
        const int nj = min(a.group, a.n_words - j0);
        for (int i = tid; i < nj * cells; i += kSwThreads) hist[i] = 0;
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            float v[kSwRun];
            sweep_expand_run(r, a.word_maps + (size_t)j * plane, a.src_w, a.out_w, v);
            if (!a.absolute) {
                const float lo = dec_ordered(a.minmax[2 * j]);
                const float hi = dec_ordered(a.minmax[2 * j + 1]);
#pragma unroll
                for (int k = 0; k < kSwRun; ++k) v[k] = (v[k] - lo) / (hi - lo + 1e-8f);
            }
            // bin = #{t : v > thr[t]}: the thresholds ascend and +inf follows them, so "v > thr[i]" holds on a prefix of i
            int bin[kSwRun] = {};
            for (int step = a.top; step > 0; step >>= 1) {
#pragma unroll
                for (int k = 0; k < kSwRun; ++k)
                    if (v[k] > thr[bin[k] + step - 1]) bin[k] += step;
            }
            uint32_t* const hj = hist + jj * cells;
#pragma unroll
            for (int k = 0; k < kSwRun; ++k) {
                unsigned long long rest = valid[k];               // wave-uniform: the pixels not yet counted
                while (rest) {
                    const int leader = __ffsll(rest) - 1;
                    const int b = __builtin_amdgcn_readlane(bin[k], leader);
                    const unsigned long long in_bin = __ballot(bin[k] == b) & rest;
                    rest &= ~in_bin;
                    const uint32_t c = (uint32_t)__popcll(in_bin & sel[k]);
                    if (lane < cols && c) atomicAdd(&hj[b * cols + lane], c);
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nj * cells; i += kSwThreads) {
            const uint32_t c = hist[i];
            if (c) atomicAdd(&a.bins[(size_t)j0 * cells + i], c);
        }
        __syncthreads();
    }
}

// one thread per (word, column): the suffix sums of its bins
__global__ __launch_bounds__(kSwThreads) void sweep_finalize_kernel(const SweepArgs a)
{
    const int cols = a.n_truth + 1;
    const int t = blockIdx.x * kSwThreads + threadIdx.x;
    if (t >= a.n_words * cols) return;
    const int j = t / cols, c = t - j * cols;
    const uint32_t* const col = a.bins + (size_t)j * (a.n_thr + 1) * cols + c;
    uint32_t* const out = c == 0 ? a.pred_area + (size_t)j * a.n_thr : a.inter + ((size_t)j * a.n_truth + (c - 1)) * a.n_thr;
    uint32_t acc = 0;
    for (int b = a.n_thr; b >= 1; --b) {
        acc += col[(size_t)b * cols];
        out[b - 1] = acc;
    }
    if (j == 0 && c > 0) a.truth_area[c - 1] = acc + col[0];     // every pixel is in exactly one bin of word 0
}

namespace {

thread_local char eval_error[256] = "";

int eval_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int eval_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(eval_error, sizeof(eval_error), fmt, ap);
    va_end(ap);
    return code;
}

bool sweep_sizes_ok(int n_words, int n_truth, int n_thr, int out_h, int out_w)
{
    return n_words >= 1 && n_words <= kSwMaxWords && n_truth >= 0 && n_truth <= kSwMaxTruth && n_thr >= 1 && n_thr <= kSwMaxThr &&
           out_h >= 1 && out_w >= 1 && (long long)out_h * out_w < (1ll << 31);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_eval_abi_version(void) { return DAAM_EVAL_ABI_VERSION; }

const char* daam_eval_last_error(void) { return eval_error; }

size_t daam_threshold_sweep_workspace(int n_words, int n_truth, int n_thr, int out_h, int out_w)
{
    if (!sweep_sizes_ok(n_words, n_truth, n_thr, out_h, out_w)) return 0;
    return kSwMinmaxBytes + (size_t)n_words * (n_thr + 1) * (n_truth + 1) * sizeof(uint32_t);
}

int daam_threshold_sweep(const float* word_maps, int n_words, int h, int w, int out_h, int out_w, int absolute, const float* thresholds,
                         int n_thr, const uint8_t* truth, int n_truth, uint32_t* pred_area, uint32_t* inter, uint32_t* truth_area,
                         void* workspace, size_t workspace_bytes, void* stream)
{
    if (!word_maps || !thresholds || !pred_area || !workspace) return eval_fail(DAAM_E_INVALID, "NULL argument");
    if (n_words < 1 || n_words > kSwMaxWords) return eval_fail(DAAM_E_INVALID, "%d words: 1..%d", n_words, kSwMaxWords);
    if (h < 1 || w < 1 || h > kSwMaxSide || w > kSwMaxSide)
        return eval_fail(DAAM_E_INVALID, "word maps of %d x %d: 1 <= h, w <= %d", h, w, kSwMaxSide);
    if (out_h < 1 || out_w < 1 || (long long)out_h * out_w >= (1ll << 31))
        return eval_fail(DAAM_E_INVALID, "output of %d x %d: at least 1 x 1, fewer than 2^31 pixels", out_h, out_w);
    if (n_thr < 1 || n_thr > kSwMaxThr) return eval_fail(DAAM_E_INVALID, "%d thresholds: 1..%d", n_thr, kSwMaxThr);
    if (n_truth < 0 || n_truth > kSwMaxTruth) return eval_fail(DAAM_E_INVALID, "%d truth masks: 0..%d", n_truth, kSwMaxTruth);
    if ((n_truth == 0) != (truth == nullptr) || (n_truth == 0) != (inter == nullptr) || (n_truth == 0) != (truth_area == nullptr))
        return eval_fail(DAAM_E_INVALID, "truth, inter and truth_area must be NULL exactly when n_truth is 0 (got %d masks)", n_truth);
    for (int t = 0; t < n_thr; ++t) {
        if (!std::isfinite(thresholds[t])) return eval_fail(DAAM_E_INVALID, "threshold %d is not finite", t);
        if (t && !(thresholds[t] > thresholds[t - 1]))
            return eval_fail(DAAM_E_INVALID, "thresholds must be strictly increasing: [%d] = %g after %g", t, thresholds[t], thresholds[t - 1]);
    }
    const size_t need = daam_threshold_sweep_workspace(n_words, n_truth, n_thr, out_h, out_w);
    if (workspace_bytes < need)
        return eval_fail(DAAM_E_INVALID, "workspace of %zu bytes: %d words, %d truth masks, %d thresholds need %zu", workspace_bytes, n_words,
                         n_truth, n_thr, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return eval_fail(DAAM_E_INVALID, "workspace is not 4-byte aligned");

    SweepArgs a;
    a.word_maps = word_maps; a.truth = truth;
    a.minmax = static_cast<int*>(workspace);
    a.bins = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(workspace) + kSwMinmaxBytes);
    a.pred_area = pred_area; a.inter = inter; a.truth_area = truth_area;
    a.n_words = n_words; a.src_h = h; a.src_w = w; a.out_h = out_h; a.out_w = out_w; a.absolute = absolute ? 1 : 0;
    a.n_thr = n_thr; a.n_truth = n_truth;
    const int cells = (n_thr + 1) * (n_truth + 1);
    a.group = kSwHistCap / cells < n_words ? kSwHistCap / cells : n_words;          // >= 5: cells <= 65 * 33
    a.top = 1;
    while (2 * a.top <= n_thr) a.top *= 2;
    for (int t = 0; t < kSwMaxThr; ++t) a.thr[t] = t < n_thr ? thresholds[t] : INFINITY;

    const hipStream_t s = (hipStream_t)stream;
    const int counters = n_words * cells;
    const long long runs = (long long)out_h * ((out_w + kSwRun - 1) / kSwRun);
    const unsigned tiles = (unsigned)((runs + kSwThreads - 1) / kSwThreads);
    const size_t lds = kSwThrSlots * sizeof(float) + (size_t)a.group * cells * sizeof(uint32_t);
    hipLaunchKernelGGL(sweep_init_kernel, dim3((counters + kSwThreads - 1) / kSwThreads), dim3(kSwThreads), 0, s, a);
    if (!absolute) hipLaunchKernelGGL(sweep_minmax_kernel, dim3(tiles), dim3(kSwThreads), 0, s, a);
    hipLaunchKernelGGL(sweep_count_kernel, dim3(tiles), dim3(kSwThreads), lds, s, a);
    hipLaunchKernelGGL(sweep_finalize_kernel, dim3((n_words * (n_truth + 1) + kSwThreads - 1) / kSwThreads), dim3(kSwThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eval_fail((int)e, "threshold sweep: %s", hipGetErrorString(e));
    return 0;
}
