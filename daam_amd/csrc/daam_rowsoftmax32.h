// What daam_self_affinity.hip and daam_joint_tap.hip share: a row softmax over K Q^T computed with
// mfma_f32_32x32x16 in two kernels -- per-row statistics (-(m c), 1 / l) from an online walk over the keys, then a second kernel that
// recomputes a tile, normalises it with the statistics and adds it up -- and the host checks of the two accumulate entry points.  Each
// file is a library of its own (one translation unit), so the host part stands in an unnamed namespace: an error buffer per library.
// A device piece is here only in a form under which every kernel of both libraries keeps its machine code, byte for byte
// (profiles/rowsoftmax_refactor.json lists the trials, tests/test_rowsoftmax_refactor_cpu.py pins the result).  The 32-key online step
// and the merge of the two lane halves are NOT here: every function form tried rescheduled the statistics kernels, so their text stands
// in both files, line for line the same.  How a tile reaches LDS, how a step is masked and where `top` starts differ on purpose.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/daam_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>

namespace daam {

constexpr int kRowMaxP = 16384;                     // rows (queries) of a slice
constexpr int kRowMaxSlices = 4096;                 // batch x heads
constexpr int kRowTile = 128;                       // query rows of a statistics block: a slice's statistics are padded to whole blocks

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

// The one read-modify-write of an element of sums at the end of the second kernel.
__device__ __forceinline__ void store_weighted(float* out, float weight, float acc, int accumulate)
{
    *out = __fmaf_rn(weight, acc, accumulate ? *out : 0.f);
}

namespace {

thread_local char last_error[256] = "";

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
    return code;
}

size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

int pad_rows(int P) { return (P + kRowTile - 1) / kRowTile * kRowTile; }

bool slices_ok(int batch, int heads) { return batch >= 1 && heads >= 1 && (long long)batch * heads <= kRowMaxSlices; }

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Bytes of the statistics of batch x heads slices of P rows; 0 when out of range.
size_t stats_workspace(int batch, int heads, int P)
{
    if (!slices_ok(batch, heads) || P < 1 || P > kRowMaxP) return 0;
    return round8(sizeof(float2) * (size_t)batch * heads * pad_rows(P));
}

// The checks of an accumulate entry point, in the order both report them; each file has checks of its own between these.  0, or the
// code that fail() returned.
int check_shape(const char* who, int in_dtype, int batch, int heads, int P)
{
    if (in_dtype != DAAM_F16 && in_dtype != DAAM_BF16) return fail(DAAM_E_INVALID, "%s: dtype %d: DAAM_F16 or DAAM_BF16", who, in_dtype);
    if (!slices_ok(batch, heads))
        return fail(DAAM_E_INVALID, "%s: batch %d x heads %d: each >= 1, at most %d slices", who, batch, heads, kRowMaxSlices);
    if (P < 1 || P > kRowMaxP) return fail(DAAM_E_INVALID, "%s: P %d: 1..%d", who, P, kRowMaxP);
    return 0;
}

int check_scale_weight(const char* who, float scale, float weight)
{
    if (!std::isfinite(scale) || !(scale > 0.f)) return fail(DAAM_E_INVALID, "%s: scale %g: finite and > 0", who, (double)scale);
    if (!std::isfinite(weight)) return fail(DAAM_E_INVALID, "%s: weight %g is not finite", who, (double)weight);
    return 0;
}

int check_outputs_and_strides(const char* who, const float* sums, const void* workspace, std::initializer_list<int64_t> strides)
{
    if (reinterpret_cast<uintptr_t>(sums) & 3) return fail(DAAM_E_INVALID, "%s: sums are not 4-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(DAAM_E_INVALID, "%s: the workspace is not 8-byte aligned", who);
    for (const int64_t st : strides)
        if (st < 0 || (st & 7) || st > ((int64_t)1 << 40))
            return fail(DAAM_E_INVALID, "%s: stride %lld: >= 0 and a multiple of 8 elements (16-byte rows)", who, (long long)st);
    return 0;
}

int check_workspace(const char* who, int batch, int heads, int P, const float* sums, size_t sums_bytes, const void* workspace,
                    size_t workspace_bytes)
{
    const size_t need = stats_workspace(batch, heads, P);
    if (workspace_bytes < need)
        return fail(DAAM_E_INVALID, "%s: workspace of %zu bytes: %d slices of %d rows need %zu", who, workspace_bytes, batch * heads, P, need);
    if (overlap(sums, sums_bytes, workspace, workspace_bytes)) return fail(DAAM_E_INVALID, "%s: sums overlap the workspace", who);
    return 0;
}

// scale log2(e), rounded once: the c of the kernels.
float log2e_scale(float scale) { return (float)((double)scale * 1.4426950408889634); }

// The tail of an entry point: 0, or the launch error as code and text.
int launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, "%s: %s", who, hipGetErrorString(e));
    return 0;
}

}  // namespace

}  // namespace daam
