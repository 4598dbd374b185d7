// daam_joint_affinity_accumulate (include/daam_joint_affinity.h): the image columns of the joint softmax of an MMDiT / FLUX attention
// call -- image queries over text AND image keys -- summed over slices into one affinity matrix f32 [P][Pk].  The row
// statistics (-(m c), 1 / l) are READ: daam_joint_tap_accumulate has just written them, or they come from anywhere else in the
// header's layout.  The MFMA wrapper, acc_row, the normalise-add (add_prob) and the weighted store are RESTATED here from the header
// that the self-affinity and the joint tap share: that header's readers are pinned to those two libraries, so this file
// reads nothing of csrc/.  add_prob must stay the expression of joint_text_kernel, term for term: a row's text and image columns
// then come from one formula and one pair of statistics.
//   * joint_image_kernel<DT, D>  : a workgroup owns a 128 x 128 tile of sums, four waves of 64 x 64 (2 x 2 MFMA blocks, queries on the
//                                  rows, image keys on the lanes so that stores run along a row of sums).  It loops over the slices
//                                  in ascending order; a slice goes through LDS in passes of 64 of depth (one with d = 64, two with
//                                  d = 128), and the NEXT pass's Q and k_img tiles and the next slice's statistics are fetched into
//                                  registers before the current pass's MFMAs and land in LDS after them.  After a slice's last
//                                  pass it adds exp2(fma(raw, c, -(m c))) * (1 / l) with one fma into 64 accumulators per lane
//                                  that stay in registers across the whole loop; one read-modify-write of sums at the end.
// Rows past P and columns past Pk are zero in LDS (their statistics (0, 0)) and are never stored.
// No atomics, no dependence on the grid: two runs give the same bits.
#include "../../include/daam_joint_affinity.h"
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kJaMaxP = 16384;                      // rows (queries) and image keys of a slice
constexpr int kJaMaxSlices = 4096;                  // batch x heads
constexpr int kJaThreads = 256;
constexpr int kJaTile = 128;                        // rows of a statistics block, rows and columns of a tile of sums

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bfloat8 __attribute__((ext_vector_type(8)));

template <int DT> struct Mma32;
template <> struct Mma32<DAAM_F16> {
    static __device__ __forceinline__ floatx16 run(const uint4& a, const uint4& b, const floatx16& c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
    }
};
template <> struct Mma32<DAAM_BF16> {
    static __device__ __forceinline__ floatx16 run(const uint4& a, const uint4& b, const floatx16& c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bfloat8, a), __builtin_bit_cast(bfloat8, b), c, 0, 0, 0);
    }
};

// The row of a 32 x 32 accumulator block that register `reg` of lane half `half` holds (the column is lane & 31).
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// acc + the probability of a raw dot product under its row's statistics st = (-(m c), 1 / l).
__device__ __forceinline__ float add_prob(float x, float c, const float2& st, float acc)
{
    return __fmaf_rn(__builtin_amdgcn_exp2f(__fmaf_rn(x, c, st.x)), st.y, acc);
}

// The one read-modify-write of an element of sums at the end of the kernel.
__device__ __forceinline__ void store_weighted(float* out, float weight, float acc, int accumulate)
{
    *out = __fmaf_rn(weight, acc, accumulate ? *out : 0.f);
}

constexpr int kJaDepth = 64;                        // depth of a pass through LDS
constexpr int kJaChunks = kJaDepth / 8;             // 16-byte chunks of a row of a pass
constexpr int kJaStage = kJaTile * kJaChunks / kJaThreads;

struct JaGeom {
    int heads, P, Pk, n_slices;
    int p_pad;                                      // P rounded up to whole tiles: the row count of a slice's statistics
    int col_tiles;                                  // tiles across Pk
    long long q_sb, q_sh, q_sp, ki_sb, ki_sh, ki_sp;
};

// A pass's tile of 128 rows x 64 of depth from depth `depth0` on, rows row0 .. of a [limit][d] matrix with row stride `stride`, as
// 16-byte chunks: chunk c of the tile (row c / 8, chunk c % 8 of the row) is thread c % 256's element c / 256 of `stage`.  Rows >= limit
// are zero.
__device__ __forceinline__ void ja_fetch(uint4 (&stage)[kJaStage], const uint16_t* __restrict__ base, long long stride, int row0,
                                         int depth0, int limit)
{
#pragma unroll
    for (int e = 0; e < kJaStage; ++e) {
        const int c = threadIdx.x + e * kJaThreads;
        const int r = c / kJaChunks, ch = c - r * kJaChunks, row = row0 + r;
        stage[e] = make_uint4(0, 0, 0, 0);
        if (row < limit) stage[e] = *reinterpret_cast<const uint4*>(base + (long long)row * stride + depth0 + ch * 8);
    }
}

// ... into LDS, 8 + 1 chunks to a row (one of padding).
__device__ __forceinline__ void ja_commit(uint4* __restrict__ lds, const uint4 (&stage)[kJaStage])
{
#pragma unroll
    for (int e = 0; e < kJaStage; ++e) {
        const int c = threadIdx.x + e * kJaThreads;
        const int r = c / kJaChunks, ch = c - r * kJaChunks;
        lds[r * (kJaChunks + 1) + ch] = stage[e];
    }
}

template <int DT, int D>
__global__ __launch_bounds__(kJaThreads) void joint_image_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_img,
                                                                 const float2* __restrict__ stats, float* __restrict__ sums, JaGeom g,
                                                                 float c, float weight, int accumulate)
{
    constexpr int CH = kJaChunks, KK = kJaDepth / 16, PASSES = D / kJaDepth;
    static_assert(D % kJaDepth == 0, "a slice is whole passes");
    __shared__ uint4 lds_q[kJaTile * (CH + 1)];
    __shared__ uint4 lds_k[kJaTile * (CH + 1)];
    __shared__ float2 lds_stat[kJaTile];
    const int ti = blockIdx.x / g.col_tiles, tj = blockIdx.x - ti * g.col_tiles;
    const int i0 = ti * kJaTile, j0 = tj * kJaTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const bool stat_row = threadIdx.x < kJaTile && i0 + threadIdx.x < g.P;      // this thread carries a row's statistics into LDS

    floatx16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = floatx16{0};

    // slice 0, pass 0
    uint4 stage_q[kJaStage], stage_k[kJaStage];
    float2 stage_st = make_float2(0.f, 0.f);
    ja_fetch(stage_q, q, g.q_sp, i0, 0, g.P);
    ja_fetch(stage_k, k_img, g.ki_sp, j0, 0, g.Pk);
    if (stat_row) stage_st = stats[i0 + threadIdx.x];
    ja_commit(lds_q, stage_q);
    ja_commit(lds_k, stage_k);
    if (threadIdx.x < kJaTile) lds_stat[threadIdx.x] = stage_st;
    __syncthreads();

    for (int s = 0; s < g.n_slices; ++s) {
        floatx16 x[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) x[mi][ni] = floatx16{0};
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            // the next pass -- of this slice, or the first of the next -- is in flight under this pass's MFMAs
            const bool last = pass + 1 == PASSES;
            const int ns = last ? s + 1 : s, ndepth = last ? 0 : (pass + 1) * kJaDepth;
            const bool more = ns < g.n_slices;
            if (more) {
                const int b = ns / g.heads, hd = ns - b * g.heads;
                ja_fetch(stage_q, q + b * g.q_sb + hd * g.q_sh, g.q_sp, i0, ndepth, g.P);
                ja_fetch(stage_k, k_img + b * g.ki_sb + hd * g.ki_sh, g.ki_sp, j0, ndepth, g.Pk);
                if (last && stat_row) stage_st = stats[(size_t)ns * g.p_pad + i0 + threadIdx.x];
            }
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                uint4 a[2], bf[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) a[mi] = lds_q[(wr * 64 + mi * 32 + r) * (CH + 1) + kk * 2 + half];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) bf[ni] = lds_k[(wc * 64 + ni * 32 + r) * (CH + 1) + kk * 2 + half];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) x[mi][ni] = Mma32<DT>::run(a[mi], bf[ni], x[mi][ni]);
            }
            if (last) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const float2 st = lds_stat[wr * 64 + mi * 32 + acc_row(reg, half)];
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) acc[mi][ni][reg] = add_prob(x[mi][ni][reg], c, st, acc[mi][ni][reg]);
                    }
            }
            __syncthreads();                        // every wave has read this pass's tiles (and, after the last, the statistics)
            if (more) {
                ja_commit(lds_q, stage_q);
                ja_commit(lds_k, stage_k);
                if (last && threadIdx.x < kJaTile) lds_stat[threadIdx.x] = stage_st;
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = i0 + wr * 64 + mi * 32 + acc_row(reg, half);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int col = j0 + wc * 64 + ni * 32 + r;
                if (row < g.P && col < g.Pk) store_weighted(sums + (size_t)row * g.Pk + col, weight, acc[mi][ni][reg], accumulate);
            }
        }
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

int pad_rows(int n) { return (n + kJaTile - 1) / kJaTile * kJaTile; }

// Bytes of the statistics of batch x heads slices of P rows; 0 when out of range.
size_t stats_bytes_of(int batch, int heads, int P)
{
    if (batch < 1 || heads < 1 || (long long)batch * heads > kJaMaxSlices || P < 1 || P > kJaMaxP) return 0;
    return sizeof(float2) * (size_t)batch * heads * pad_rows(P);
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <int DT, int D>
void launch(hipStream_t s, const void* q, const void* k_img, const float2* stats, float* sums, const JaGeom& g, float c, float weight,
            int accumulate)
{
    const unsigned tiles = (unsigned)(g.p_pad / kJaTile) * (unsigned)g.col_tiles;
    hipLaunchKernelGGL((joint_image_kernel<DT, D>), dim3(tiles), dim3(kJaThreads), 0, s, static_cast<const uint16_t*>(q),
                       static_cast<const uint16_t*>(k_img), stats, sums, g, c, weight, accumulate);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_joint_affinity_abi_version(void) { return DAAM_JOINT_AFFINITY_ABI_VERSION; }

const char* daam_joint_affinity_last_error(void) { return last_error; }

size_t daam_joint_affinity_stats_bytes(int batch, int heads, int P) { return stats_bytes_of(batch, heads, P); }

int daam_joint_affinity_accumulate(const void* q, const void* k_img, const void* stats, size_t stats_bytes, int in_dtype, int batch,
                                   int heads, int P, int Pk, int d, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p,
                                   int64_t ki_stride_b, int64_t ki_stride_h, int64_t ki_stride_p, float scale, float weight, int accumulate,
                                   float* sums, void* stream)
{
    const char* who = "joint_affinity_accumulate";
    if (in_dtype != DAAM_F16 && in_dtype != DAAM_BF16) return fail("%s: dtype %d: fp16 (DAAM_F16) or bf16 (DAAM_BF16)", who, in_dtype);
    if (batch < 1 || heads < 1 || (long long)batch * heads > kJaMaxSlices)
        return fail("%s: batch %d x heads %d: each >= 1 and no more than %d slices", who, batch, heads, kJaMaxSlices);
    if (P < 1 || P > kJaMaxP) return fail("%s: P %d: 1..%d", who, P, kJaMaxP);
    if (Pk < 1 || Pk > kJaMaxP) return fail("%s: Pk %d: 1..%d", who, Pk, kJaMaxP);
    if (d != 64 && d != 128) return fail("%s: head dim %d: 64 or 128", who, d);
    if (!std::isfinite(scale) || !(scale > 0.f)) return fail("%s: scale %g: a finite number above 0", who, (double)scale);
    if (!std::isfinite(weight)) return fail("%s: weight %g: a finite number", who, (double)weight);
    if (!q || !k_img || !stats || !sums) return fail("%s: q, k_img, stats and sums must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_img)) & 15) return fail("%s: q and k_img must be 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(stats) & 7) return fail("%s: stats must be 8-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(sums) & 3) return fail("%s: sums must be 4-byte aligned", who);
    for (const int64_t st : {q_stride_b, q_stride_h, q_stride_p, ki_stride_b, ki_stride_h, ki_stride_p})
        if (st < 0 || (st & 7) || st > ((int64_t)1 << 40))
            return fail("%s: stride %lld: >= 0 and whole 16-byte rows (8 elements)", who, (long long)st);
    if (q_stride_p < d || ki_stride_p < d)
        return fail("%s: row strides %lld / %lld below the head dim %d", who, (long long)q_stride_p, (long long)ki_stride_p, d);
    const size_t need = stats_bytes_of(batch, heads, P);
    if (stats_bytes < need) return fail("%s: stats of %zu bytes: %d slices x %d rows take %zu", who, stats_bytes, batch * heads, P, need);
    if (overlap(sums, sizeof(float) * (size_t)P * Pk, stats, stats_bytes)) return fail("%s: stats overlap sums", who);

    JaGeom g;
    g.heads = heads; g.P = P; g.Pk = Pk; g.n_slices = batch * heads; g.p_pad = pad_rows(P); g.col_tiles = pad_rows(Pk) / kJaTile;
    g.q_sb = q_stride_b; g.q_sh = q_stride_h; g.q_sp = q_stride_p;
    g.ki_sb = ki_stride_b; g.ki_sh = ki_stride_h; g.ki_sp = ki_stride_p;
    const float c = (float)((double)scale * 1.4426950408889634);        // scale log2(e), rounded once: the c of the statistics
    const hipStream_t s = (hipStream_t)stream;
    const float2* const st = static_cast<const float2*>(stats);
    const int acc = accumulate != 0;
    if (in_dtype == DAAM_F16) {
        if (d == 64) launch<DAAM_F16, 64>(s, q, k_img, st, sums, g, c, weight, acc);
        else launch<DAAM_F16, 128>(s, q, k_img, st, sums, g, c, weight, acc);
    } else {
        if (d == 64) launch<DAAM_BF16, 64>(s, q, k_img, st, sums, g, c, weight, acc);
        else launch<DAAM_BF16, 128>(s, q, k_img, st, sums, g, c, weight, acc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fail("%s: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}
