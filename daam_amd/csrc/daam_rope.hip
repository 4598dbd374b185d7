// daam_rope_apply (include/daam_rope.h): the rotary embedding of a FLUX-class attention call on up to four tensors in one launch
// (DESIGN 3.25).  Memory-bound, no LDS:
//   * rope_kernel<DT, D>  : a lane owns 8 consecutive elements (4 interleaved pairs) of one (batch, row, head): one 16-byte load of x,
//                           32 bytes of cos and of sin, 16 f32 multiplies and 8 adds (none contracted), one 16-byte store.  Lanes run
//                           along d, then the heads, then rows, then the batch, so that in the layout of the projections
//                           ([batch, rows, heads d]) a wave reads and writes whole 128-byte lines; the cos / sin of a row are read
//                           again by every head, out of L2.  Jobs lie end to end over the grid: a workgroup finds its job by
//                           comparing its index with three prefix counts that travel in the kernel argument.  The last workgroup
//                           of a job masks its tail; nothing is padded.
// No atomics, no scratch, no dependence on the grid: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/daam_rope.h"

#include <cstdarg>
#include <cstdio>

#pragma clang fp contract(off)                      // no product of this file may be fused into an fma (fmul / fadd below)

namespace daam {

constexpr int kRopeThreads = 256;
constexpr int kRopeLane = 8;                        // elements a lane owns

struct RopeJobArg {
    const uint16_t* x;
    uint16_t* out;
    const float* cos;
    const float* sin;
    long long x_sb, x_sr, x_sh, o_sb, o_sr, o_sh, table_stride;
    unsigned rows, heads, items;                    // items = batch * rows * heads * (D / 8) < 2^32 (4096 * 16896 * 16)
    unsigned first_block;                           // workgroups of the jobs before this one
};

struct RopeArgs {
    RopeJobArg job[DAAM_ROPE_MAX_JOBS];             // jobs past n_jobs repeat the last one's first_block + blocks: never selected
};

template <int DT> struct RopeElem;
template <> struct RopeElem<DAAM_F16> {
    static __device__ __forceinline__ float load(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
    static __device__ __forceinline__ unsigned round(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }      // v_cvt_f16_f32: RNE
};
template <> struct RopeElem<DAAM_BF16> {
    static __device__ __forceinline__ float load(unsigned bits) { return __uint_as_float(bits << 16); }
    static __device__ __forceinline__ unsigned round(float v)
    {
        const unsigned u = __float_as_uint(v);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;          // NaN stays NaN (quiet)
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                          // nearest, ties to even; carries into +-inf
    }
};

// One IEEE f32 operation each.  They are written here, under the pragma above, and not taken from the HIP headers: __fmul_rn and
// __fadd_rn are plain `*` and `+` compiled under the headers' own contraction mode, and hipcc fuses a pair of them into v_fma_f32.
__device__ __forceinline__ float fmul(float a, float b) { return a * b; }
__device__ __forceinline__ float fadd(float a, float b) { return a + b; }

template <int DT>
__device__ __forceinline__ unsigned rope_pair(unsigned word, float c0, float c1, float s0, float s1)
{
    const float a = RopeElem<DT>::load(word & 0xFFFFu), b = RopeElem<DT>::load(word >> 16);
    const float even = fadd(fmul(a, c0), fmul(-b, s0));
    const float odd = fadd(fmul(b, c1), fmul(a, s1));
    return RopeElem<DT>::round(even) | (RopeElem<DT>::round(odd) << 16);
}

template <int DT, int D>
__global__ __launch_bounds__(kRopeThreads) void rope_kernel(const RopeArgs args)
{
    constexpr unsigned kLanes = D / kRopeLane;      // lanes of one head
    const unsigned block = blockIdx.x;
    const int j = (int)(block >= args.job[1].first_block) + (int)(block >= args.job[2].first_block) + (int)(block >= args.job[3].first_block);
    const RopeJobArg& g = args.job[j];
    const unsigned item = (block - g.first_block) * kRopeThreads + threadIdx.x;
    if (item >= g.items) return;
    const unsigned c = item % kLanes, bh = item / kLanes;
    const unsigned h = bh % g.heads, br = bh / g.heads;
    const unsigned r = br % g.rows, b = br / g.rows;
    const uint4 xv = *reinterpret_cast<const uint4*>(g.x + b * g.x_sb + r * g.x_sr + h * g.x_sh + c * kRopeLane);
    const float4* const cp = reinterpret_cast<const float4*>(g.cos + r * g.table_stride + c * kRopeLane);
    const float4* const sp = reinterpret_cast<const float4*>(g.sin + r * g.table_stride + c * kRopeLane);
    const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
    uint4 ov;
    ov.x = rope_pair<DT>(xv.x, c0.x, c0.y, s0.x, s0.y);
    ov.y = rope_pair<DT>(xv.y, c0.z, c0.w, s0.z, s0.w);
    ov.z = rope_pair<DT>(xv.z, c1.x, c1.y, s1.x, s1.y);
    ov.w = rope_pair<DT>(xv.w, c1.z, c1.w, s1.z, s1.w);
    *reinterpret_cast<uint4*>(g.out + b * g.o_sb + r * g.o_sr + h * g.o_sh + c * kRopeLane) = ov;
}

namespace {

thread_local char rope_error[256] = "";

int rope_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int rope_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(rope_error, sizeof(rope_error), fmt, ap);
    va_end(ap);
    return code;
}

// elements from the first to one past the last a job touches in a tensor of these strides
int64_t extent(const daam_rope_job& j, int64_t sb, int64_t sr, int64_t sh, int d)
{
    return (j.batch - 1) * sb + (j.rows - 1) * sr + (j.heads - 1) * sh + d;
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_rope_abi_version(void) { return DAAM_ROPE_ABI_VERSION; }

const char* daam_rope_last_error(void) { return rope_error; }

int daam_rope_apply(const daam_rope_job* jobs, int n_jobs, int dtype, int d, void* stream)
{
    const char* who = "rope_apply";
    if (n_jobs < 1 || n_jobs > DAAM_ROPE_MAX_JOBS) return rope_fail(DAAM_E_INVALID, "%s: %d jobs: 1..%d", who, n_jobs, DAAM_ROPE_MAX_JOBS);
    if (!jobs) return rope_fail(DAAM_E_INVALID, "%s: jobs must not be NULL", who);
    if (dtype != DAAM_F16 && dtype != DAAM_BF16) return rope_fail(DAAM_E_INVALID, "%s: dtype %d: DAAM_F16 or DAAM_BF16", who, dtype);
    if (d != 64 && d != 128) return rope_fail(DAAM_E_INVALID, "%s: head dim %d: 64 or 128", who, d);
    RopeArgs args;
    unsigned blocks = 0;
    for (int n = 0; n < n_jobs; ++n) {
        const daam_rope_job& j = jobs[n];
        if (!j.x || !j.out || !j.cos || !j.sin) return rope_fail(DAAM_E_INVALID, "%s: job %d: x, out, cos and sin must not be NULL", who, n);
        if (j.batch < 1 || j.heads < 1 || (long long)j.batch * j.heads > DAAM_ROPE_MAX_SLICES)
            return rope_fail(DAAM_E_INVALID, "%s: job %d: batch %d x heads %d: each >= 1, at most %d slices", who, n, j.batch, j.heads,
                             DAAM_ROPE_MAX_SLICES);
        if (j.rows < 1 || j.rows > DAAM_ROPE_MAX_ROWS) return rope_fail(DAAM_E_INVALID, "%s: job %d: rows %d: 1..%d", who, n, j.rows, DAAM_ROPE_MAX_ROWS);
        if ((reinterpret_cast<uintptr_t>(j.x) | reinterpret_cast<uintptr_t>(j.out)) & 15)
            return rope_fail(DAAM_E_INVALID, "%s: job %d: x and out must be 16-byte aligned", who, n);
        if ((reinterpret_cast<uintptr_t>(j.cos) | reinterpret_cast<uintptr_t>(j.sin)) & 15)
            return rope_fail(DAAM_E_INVALID, "%s: job %d: cos and sin must be 16-byte aligned", who, n);
        const int64_t strides[] = {j.x_stride_b, j.x_stride_r, j.x_stride_h, j.out_stride_b, j.out_stride_r, j.out_stride_h};
        for (const int64_t st : strides)
            if (st < 0 || (st & 7) || st > ((int64_t)1 << 40))
                return rope_fail(DAAM_E_INVALID, "%s: job %d: stride %lld: >= 0 and a multiple of 8 elements (16-byte rows)", who, n, (long long)st);
        if (j.x_stride_r < d || j.x_stride_h < d || j.out_stride_r < d || j.out_stride_h < d)
            return rope_fail(DAAM_E_INVALID, "%s: job %d: row / head strides %lld / %lld (x), %lld / %lld (out) below the head dim %d", who, n,
                             (long long)j.x_stride_r, (long long)j.x_stride_h, (long long)j.out_stride_r, (long long)j.out_stride_h, d);
        if (j.table_stride < d || (j.table_stride & 3) || j.table_stride > ((int64_t)1 << 40))
            return rope_fail(DAAM_E_INVALID, "%s: job %d: table_stride %lld: >= d = %d and a multiple of 4 floats", who, n, (long long)j.table_stride, d);
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(j.x), o0 = reinterpret_cast<uintptr_t>(j.out);
        const uint64_t x_bytes = 2 * (uint64_t)extent(j, j.x_stride_b, j.x_stride_r, j.x_stride_h, d);
        const uint64_t o_bytes = 2 * (uint64_t)extent(j, j.out_stride_b, j.out_stride_r, j.out_stride_h, d);
        if (x0 < o0 + o_bytes && o0 < x0 + x_bytes) return rope_fail(DAAM_E_INVALID, "%s: job %d: out overlaps x", who, n);
        RopeJobArg& a = args.job[n];
        a.x = static_cast<const uint16_t*>(j.x); a.out = static_cast<uint16_t*>(j.out); a.cos = j.cos; a.sin = j.sin;
        a.x_sb = j.x_stride_b; a.x_sr = j.x_stride_r; a.x_sh = j.x_stride_h;
        a.o_sb = j.out_stride_b; a.o_sr = j.out_stride_r; a.o_sh = j.out_stride_h; a.table_stride = j.table_stride;
        a.rows = (unsigned)j.rows; a.heads = (unsigned)j.heads;
        a.items = (unsigned)j.batch * (unsigned)j.rows * (unsigned)j.heads * (unsigned)(d / kRopeLane);
        a.first_block = blocks;
        blocks += (a.items + kRopeThreads - 1) / kRopeThreads;
    }
    for (int n = n_jobs; n < DAAM_ROPE_MAX_JOBS; ++n) {
        args.job[n] = args.job[n_jobs - 1];
        args.job[n].first_block = blocks;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == DAAM_F16) {
        if (d == 64) hipLaunchKernelGGL((rope_kernel<DAAM_F16, 64>), dim3(blocks), dim3(kRopeThreads), 0, s, args);
        else hipLaunchKernelGGL((rope_kernel<DAAM_F16, 128>), dim3(blocks), dim3(kRopeThreads), 0, s, args);
    } else {
        if (d == 64) hipLaunchKernelGGL((rope_kernel<DAAM_BF16, 64>), dim3(blocks), dim3(kRopeThreads), 0, s, args);
        else hipLaunchKernelGGL((rope_kernel<DAAM_BF16, 128>), dim3(blocks), dim3(kRopeThreads), 0, s, args);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rope_fail((int)e, "%s: %s", who, hipGetErrorString(e));
    return 0;
}
