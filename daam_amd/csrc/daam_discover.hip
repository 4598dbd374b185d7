// libdaam_discover.so (include/daam_discover.h): segments from a self-affinity without a word list.  Four stateless passes:
//   * discover_prepare_kernel : a workgroup per row.  Thread t adds cells t, t + 256, ... ascending, the 256 partial sums are added
//                               pairwise through LDS (m = 128, 64, ..., 1); then p = src / sum and l = logf(max(p, 2^-120)).
//   * discover_pair_kl_kernel : the hot one, VALU work that is no GEMM.  A workgroup of 256 lanes owns a 64 x 64 tile of D, a lane the
//                               4 x 4 outputs (ta + 16 i, tb + 16 i').  Both operands (P and L of either side) walk along j through
//                               LDS in chunks of 32 cells, rows 36 floats apart: a lane reads a float4 of four consecutive cells of
//                               each of its 4 + 4 rows of P and of L (16 ds_read_b128) and spends them on 64 terms (192 VALU
//                               instructions).  The 16 lanes of a read group hold 16 consecutive rows, 36 floats apart: 16 distinct
//                               4-bank slots, no conflict; lanes that share a row share the address.  LDS is double-buffered: the
//                               NEXT chunk's global loads are issued into 8 float4 registers before the current chunk's arithmetic
//                               and land in the other buffer after it, one barrier per chunk.  acc = fma(pa - pb, la - lb, acc), j
//                               ascending within every accumulator.  Rows past A / B and cells past N are zero in LDS and are never
//                               stored.  VEC: float4 global loads when N is a multiple of 4 and the four bases are 16-byte aligned.
//   * discover_merge_kernel   : a workgroup per (256 cells, k): the membership row goes through LDS as words of four flags, every lane
//                               adds the member rows of its cell in ascending r and divides by the count.
//   * discover_labels_kernel  : a lane per output pixel: tap positions and weights from integers, the four-tap value of every proposal
//                               in ascending k, the first largest kept.
// No atomics, no scratch, no dependence on the grid: two runs give the same bits.
#include "../../include/daam_discover.h"
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kDiMaxRows = 16384;                   // R, A, B
constexpr int kDiMaxCells = 16384;                  // N
constexpr int kDiMaxGroups = 1024;                  // K of merge
constexpr int kDiMaxProps = 255;                    // K of labels
constexpr int kDiMaxGrid = 128;                     // h, w of labels
constexpr int kDiMaxOut = 2048;                     // out_h, out_w of labels
constexpr int kDiThreads = 256;
constexpr float kDiEps = 0x1p-120f;

// ---- prepare ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDiThreads) void discover_prepare_kernel(const float* __restrict__ src, long long stride, int N,
                                                                      float* __restrict__ P, float* __restrict__ L)
{
    __shared__ float part[kDiThreads];
    const float* row = src + (long long)blockIdx.x * stride;
    const int t = threadIdx.x;
    float s = 0.f;
    for (int j = t; j < N; j += kDiThreads) s = __fadd_rn(s, row[j]);
    part[t] = s;
    __syncthreads();
#pragma unroll
    for (int m = kDiThreads / 2; m >= 1; m >>= 1) {
        if (t < m) part[t] = __fadd_rn(part[t], part[t + m]);
        __syncthreads();
    }
    const float sum = part[0];
    const bool ok = sum != 0.f && isfinite(sum);
    float* p_row = P + (size_t)blockIdx.x * N;
    float* l_row = L + (size_t)blockIdx.x * N;
    for (int j = t; j < N; j += kDiThreads) {
        const float p = ok ? __fdiv_rn(row[j], sum) : 0.f;
        p_row[j] = p;
        l_row[j] = logf(fmaxf(p, kDiEps));
    }
}

// ---- pair_kl ---------------------------------------------------------------------------------------------------------------------------
constexpr int kKlTile = 64;                         // rows of Pa / Pb of a tile of D
constexpr int kKlChunk = 32;                        // cells of a chunk
constexpr int kKlStride = kKlChunk + 4;             // floats between rows in LDS
constexpr int kKlQuads = kKlTile * kKlChunk / 4 / kDiThreads;      // float4 a lane stages per operand and chunk
constexpr int kKlPlane = kKlTile * kKlStride;       // floats of one operand's chunk in LDS

// Quad q of lane's share of a chunk: row q / 8, cells 4 (q % 8) .. + 3 of the chunk that starts at cell j0.
template <bool VEC>
__device__ __forceinline__ float4 kl_load(const float* __restrict__ base, int row, int rows, int j, int N)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows) {
        const float* p = base + (size_t)row * N + j;
        if (VEC) {
            if (j < N) v = *reinterpret_cast<const float4*>(p);
        } else {
            if (j < N) v.x = p[0];
            if (j + 1 < N) v.y = p[1];
            if (j + 2 < N) v.z = p[2];
            if (j + 3 < N) v.w = p[3];
        }
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void kl_fetch(float4 (&stage)[4][kKlQuads], const float* __restrict__ Pa, const float* __restrict__ La,
                                         const float* __restrict__ Pb, const float* __restrict__ Lb, int a0, int b0, int A, int B, int j0,
                                         int N)
{
#pragma unroll
    for (int e = 0; e < kKlQuads; ++e) {
        const int q = threadIdx.x + e * kDiThreads;
        const int r = q >> 3, j = j0 + 4 * (q & 7);
        stage[0][e] = kl_load<VEC>(Pa, a0 + r, A, j, N);
        stage[1][e] = kl_load<VEC>(La, a0 + r, A, j, N);
        stage[2][e] = kl_load<VEC>(Pb, b0 + r, B, j, N);
        stage[3][e] = kl_load<VEC>(Lb, b0 + r, B, j, N);
    }
}

__device__ __forceinline__ void kl_commit(float* __restrict__ buf, const float4 (&stage)[4][kKlQuads])
{
#pragma unroll
    for (int op = 0; op < 4; ++op)
#pragma unroll
        for (int e = 0; e < kKlQuads; ++e) {
            const int q = threadIdx.x + e * kDiThreads;
            *reinterpret_cast<float4*>(buf + op * kKlPlane + (q >> 3) * kKlStride + 4 * (q & 7)) = stage[op][e];
        }
}

__device__ __forceinline__ float kl_at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

template <bool VEC>
__global__ __launch_bounds__(kDiThreads) void discover_pair_kl_kernel(const float* __restrict__ Pa, const float* __restrict__ La, int A,
                                                                      const float* __restrict__ Pb, const float* __restrict__ Lb, int B,
                                                                      int N, float* __restrict__ D)
{
    __shared__ __attribute__((aligned(16))) float lds[2][4 * kKlPlane];
    const int a0 = blockIdx.y * kKlTile, b0 = blockIdx.x * kKlTile;
    const int tb = threadIdx.x & 15, ta = threadIdx.x >> 4;
    const int chunks = (N + kKlChunk - 1) / kKlChunk;

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;

    float4 stage[4][kKlQuads];
    kl_fetch<VEC>(stage, Pa, La, Pb, Lb, a0, b0, A, B, 0, N);
    kl_commit(lds[0], stage);
    __syncthreads();

    for (int c = 0; c < chunks; ++c) {
        const bool more = c + 1 < chunks;
        if (more) kl_fetch<VEC>(stage, Pa, La, Pb, Lb, a0, b0, A, B, (c + 1) * kKlChunk, N);      // in flight under the arithmetic
        const float* buf = lds[c & 1];
#pragma unroll 2
        for (int jq = 0; jq < kKlChunk / 4; ++jq) {
            float4 pa[4], la[4], pb[4], lb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pa[i] = *reinterpret_cast<const float4*>(buf + 0 * kKlPlane + (ta + 16 * i) * kKlStride + 4 * jq);
                la[i] = *reinterpret_cast<const float4*>(buf + 1 * kKlPlane + (ta + 16 * i) * kKlStride + 4 * jq);
                pb[i] = *reinterpret_cast<const float4*>(buf + 2 * kKlPlane + (tb + 16 * i) * kKlStride + 4 * jq);
                lb[i] = *reinterpret_cast<const float4*>(buf + 3 * kKlPlane + (tb + 16 * i) * kKlStride + 4 * jq);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)                      // j ascending within every accumulator
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        acc[i][k] = __fmaf_rn(__fsub_rn(kl_at(pa[i], e), kl_at(pb[k], e)), __fsub_rn(kl_at(la[i], e), kl_at(lb[k], e)),
                                              acc[i][k]);
        }
        if (more) kl_commit(lds[(c + 1) & 1], stage);      // the buffer chunk c - 1 was read from: every wave passed the barrier since
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = a0 + ta + 16 * i;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = b0 + tb + 16 * k;
            if (a < A && b < B) D[(size_t)a * B + b] = 0.5f * acc[i][k];
        }
    }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDiThreads) void discover_merge_kernel(const float* __restrict__ P, int R, int N,
                                                                    const uint8_t* __restrict__ member, float* __restrict__ out,
                                                                    int32_t* __restrict__ cnt)
{
    __shared__ uint32_t flags[kDiMaxRows / 4];
    const int k = blockIdx.y, j = blockIdx.x * kDiThreads + threadIdx.x;
    const uint8_t* row = member + (size_t)k * R;
    const int words = (R + 3) / 4;
    for (int wd = threadIdx.x; wd < words; wd += kDiThreads) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * wd + e < R && row[4 * wd + e]) v |= 1u << (8 * e);
        flags[wd] = v;
    }
    __syncthreads();
    float s = 0.f;
    int n = 0;
    for (int wd = 0; wd < words; ++wd) {
        const uint32_t v = flags[wd];
        if (!v) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v & (1u << (8 * e))) {                       // r ascending
                ++n;
                if (j < N) s = __fadd_rn(s, P[(size_t)(4 * wd + e) * N + j]);
            }
    }
    if (j < N) out[(size_t)k * N + j] = n ? __fdiv_rn(s, (float)n) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[k] = n;
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------------
// Tap positions and weights of output index o of `out` along an axis of `in` cells: the source position ((2 o + 1) in - out) / (2 out),
// clamped at 0, split into its floor and the two weights (den - r) / den and r / den, each one rounding of a ratio of integers.
__device__ __forceinline__ void label_taps(int o, int in, int out, int& i0, int& i1, float& w0, float& w1)
{
    const int den = 2 * out;
    int num = (2 * o + 1) * in - out;
    if (num < 0) num = 0;
    i0 = num / den;
    const int r = num - i0 * den;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    w1 = __fdiv_rn((float)r, (float)den);
    w0 = __fdiv_rn((float)(den - r), (float)den);
}

__global__ __launch_bounds__(kDiThreads) void discover_labels_kernel(const float* __restrict__ props, int K, int h, int w, int out_h,
                                                                     int out_w, uint8_t* __restrict__ labels, float* __restrict__ values)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || y >= out_h) return;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    label_taps(y, h, out_h, y0, y1, wy0, wy1);
    label_taps(x, w, out_w, x0, x1, wx0, wx1);
    const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
    float best = 0.f;
    int label = 0;
    for (int k = 0; k < K; ++k) {
        const float* p = props + (size_t)k * h * w;
        const float top = __fmaf_rn(wx1, p[o01], __fmul_rn(wx0, p[o00]));
        const float bot = __fmaf_rn(wx1, p[o11], __fmul_rn(wx0, p[o10]));
        const float v = __fmaf_rn(wy1, bot, __fmul_rn(wy0, top));
        if (k == 0 || v > best) {                            // a tie stays with the lowest index
            best = v;
            label = k;
        }
    }
    labels[(size_t)y * out_w + x] = (uint8_t)label;
    if (values) values[(size_t)y * out_w + x] = best;
}

namespace {

thread_local char last_error[256] = "";

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
    return DAAM_E_INVALID;
}

struct Span {
    const void* p;
    size_t bytes;
    const char* name;
};

bool overlap(const Span& a, const Span& b)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// No NULL, 4-byte alignment (but for spans of bytes, align 1), and no output over an input or another output.
template <size_t NI, size_t NO>
int check_spans(const char* who, const Span (&in)[NI], const Span (&out)[NO], const size_t (&out_align)[NO])
{
    for (const Span& s : in)
        if (!s.p) return fail("%s: %s must not be NULL", who, s.name);
    for (const Span& s : out)
        if (!s.p) return fail("%s: %s must not be NULL", who, s.name);
    for (size_t o = 0; o < NO; ++o) {
        if (reinterpret_cast<uintptr_t>(out[o].p) & (out_align[o] - 1))
            return fail("%s: %s must be %zu-byte aligned", who, out[o].name, out_align[o]);
        for (const Span& s : in)
            if (overlap(out[o], s)) return fail("%s: %s overlaps %s", who, out[o].name, s.name);
        for (size_t o2 = o + 1; o2 < NO; ++o2)
            if (overlap(out[o], out[o2])) return fail("%s: %s overlaps %s", who, out[o].name, out[o2].name);
    }
    return 0;
}

bool aligned4(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 3); }

int launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fail("%s: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_discover_abi_version(void) { return DAAM_DISCOVER_ABI_VERSION; }

const char* daam_discover_last_error(void) { return last_error; }

int daam_discover_prepare(const float* src, int64_t src_stride, int R, int N, float* P, float* L, void* stream)
{
    const char* who = "discover_prepare";
    if (R < 1 || R > kDiMaxRows) return fail("%s: R %d: 1..%d", who, R, kDiMaxRows);
    if (N < 1 || N > kDiMaxCells) return fail("%s: N %d: 1..%d", who, N, kDiMaxCells);
    if (src_stride < N || src_stride > ((int64_t)1 << 40)) return fail("%s: row stride %lld below N %d", who, (long long)src_stride, N);
    const size_t bytes = sizeof(float) * (size_t)R * N;
    const Span in[] = {{src, sizeof(float) * ((size_t)(R - 1) * src_stride + N), "src"}};
    const Span out[] = {{P, bytes, "P"}, {L, bytes, "L"}};
    if (const int rc = check_spans(who, in, out, {4, 4})) return rc;
    if (!aligned4(src)) return fail("%s: src must be 4-byte aligned", who);
    hipLaunchKernelGGL(discover_prepare_kernel, dim3(R), dim3(kDiThreads), 0, (hipStream_t)stream, src, (long long)src_stride, N, P, L);
    return launched(who);
}

int daam_discover_pair_kl(const float* Pa, const float* La, int A, const float* Pb, const float* Lb, int B, int N, float* D, void* stream)
{
    const char* who = "discover_pair_kl";
    if (A < 1 || A > kDiMaxRows) return fail("%s: A %d: 1..%d", who, A, kDiMaxRows);
    if (B < 1 || B > kDiMaxRows) return fail("%s: B %d: 1..%d", who, B, kDiMaxRows);
    if (N < 1 || N > kDiMaxCells) return fail("%s: N %d: 1..%d", who, N, kDiMaxCells);
    const size_t a_bytes = sizeof(float) * (size_t)A * N, b_bytes = sizeof(float) * (size_t)B * N;
    const Span in[] = {{Pa, a_bytes, "Pa"}, {La, a_bytes, "La"}, {Pb, b_bytes, "Pb"}, {Lb, b_bytes, "Lb"}};
    const Span out[] = {{D, sizeof(float) * (size_t)A * B, "D"}};
    if (const int rc = check_spans(who, in, out, {4})) return rc;
    for (const Span& s : in)
        if (!aligned4(s.p)) return fail("%s: %s must be 4-byte aligned", who, s.name);
    const bool vec = N % 4 == 0 && !((reinterpret_cast<uintptr_t>(Pa) | reinterpret_cast<uintptr_t>(La) | reinterpret_cast<uintptr_t>(Pb) |
                                      reinterpret_cast<uintptr_t>(Lb)) & 15);
    const dim3 grid((B + kKlTile - 1) / kKlTile, (A + kKlTile - 1) / kKlTile);
    if (vec) hipLaunchKernelGGL(discover_pair_kl_kernel<true>, grid, dim3(kDiThreads), 0, (hipStream_t)stream, Pa, La, A, Pb, Lb, B, N, D);
    else hipLaunchKernelGGL(discover_pair_kl_kernel<false>, grid, dim3(kDiThreads), 0, (hipStream_t)stream, Pa, La, A, Pb, Lb, B, N, D);
    return launched(who);
}

int daam_discover_merge(const float* P, int R, int N, const uint8_t* member, int K, float* out, int32_t* cnt, void* stream)
{
    const char* who = "discover_merge";
    if (R < 1 || R > kDiMaxRows) return fail("%s: R %d: 1..%d", who, R, kDiMaxRows);
    if (N < 1 || N > kDiMaxCells) return fail("%s: N %d: 1..%d", who, N, kDiMaxCells);
    if (K < 1 || K > kDiMaxGroups) return fail("%s: K %d: 1..%d", who, K, kDiMaxGroups);
    const Span in[] = {{P, sizeof(float) * (size_t)R * N, "P"}, {member, (size_t)K * R, "member"}};
    const Span outs[] = {{out, sizeof(float) * (size_t)K * N, "out"}, {cnt, sizeof(int32_t) * (size_t)K, "cnt"}};
    if (const int rc = check_spans(who, in, outs, {4, 4})) return rc;
    if (!aligned4(P)) return fail("%s: P must be 4-byte aligned", who);
    hipLaunchKernelGGL(discover_merge_kernel, dim3((N + kDiThreads - 1) / kDiThreads, K), dim3(kDiThreads), 0, (hipStream_t)stream, P, R, N,
                       member, out, cnt);
    return launched(who);
}

int daam_discover_labels(const float* props, int K, int h, int w, int out_h, int out_w, uint8_t* labels, float* values, void* stream)
{
    const char* who = "discover_labels";
    if (K < 1 || K > kDiMaxProps) return fail("%s: K %d: 1..%d", who, K, kDiMaxProps);
    if (h < 1 || h > kDiMaxGrid || w < 1 || w > kDiMaxGrid) return fail("%s: grid %d x %d: each 1..%d", who, h, w, kDiMaxGrid);
    if (out_h < 1 || out_h > kDiMaxOut || out_w < 1 || out_w > kDiMaxOut)
        return fail("%s: output %d x %d: each 1..%d", who, out_h, out_w, kDiMaxOut);
    const size_t pixels = (size_t)out_h * out_w;
    const Span in[] = {{props, sizeof(float) * (size_t)K * h * w, "props"}};
    if (!aligned4(props)) return fail("%s: props must be 4-byte aligned", who);
    if (values) {
        const Span outs[] = {{labels, pixels, "labels"}, {values, sizeof(float) * pixels, "values"}};
        if (const int rc = check_spans(who, in, outs, {1, 4})) return rc;
    } else {
        const Span outs[] = {{labels, pixels, "labels"}};
        if (const int rc = check_spans(who, in, outs, {1})) return rc;
    }
    hipLaunchKernelGGL(discover_labels_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(kDiThreads), 0, (hipStream_t)stream, props, K,
                       h, w, out_h, out_w, labels, values);
    return launched(who);
}
