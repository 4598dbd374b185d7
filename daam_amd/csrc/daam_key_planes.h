// What the per-key analyses of libdaam_analysis.so (include/daam_analysis.h) share: daam_key_scores.h, daam_token_gram.h and
// daam_key_blend.h include this header, and each keeps only what is its own.  A key is a DaamKeyPlanes; here are its limits and "is it a plane", its element
// types, and the host's one error buffer and one wording of the argument checks every entry point makes (both defined in
// daam_key_scores.hip, which also holds daam_analysis_last_error).
#pragma once
#include "daam_finalize.h"                       // float4v / floatx16 / half8 / ushort8, fin_dispatch, fin_launch
#include "../../include/daam_analysis.h"

namespace daam {

constexpr int kKeyMaxSide = 128;
constexpr int kKeyMaxKeys = 1 << 20;

// a key that is not a plane is not read: its results are NaN
__host__ __device__ inline bool key_planes_ok(const DaamKeyPlanes& k)
{
    return k.h >= 1 && k.h <= kKeyMaxSide && k.w >= 1 && k.w <= kKeyMaxSide && k.n_win >= 1;
}

// a plane element type: its 16-byte piece, and the element as f32
template <typename T> struct KeyElem;
template <> struct KeyElem<_Float16> {
    static constexpr int E = 8;
    using Piece = half8;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return (float)p[i]; }
    static __device__ __forceinline__ float one(const _Float16* s) { return (float)*as_global<_Float16>(s); }
};
template <> struct KeyElem<bf16_t> {
    static constexpr int E = 8;
    using Piece = ushort8;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return __uint_as_float((unsigned)p[i] << 16); }
    static __device__ __forceinline__ float one(const bf16_t* s) { return __uint_as_float((unsigned)*as_global<unsigned short>(s) << 16); }
};
template <> struct KeyElem<float> {
    static constexpr int E = 4;
    using Piece = float4v;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return p[i]; }
    static __device__ __forceinline__ float one(const float* s) { return *as_global<float>(s); }
};

// host: the message daam_analysis_last_error() returns on this thread; returns `code`
int analysis_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// host: the checks every entry point makes before any HIP call -- 1 <= n_keys <= kKeyMaxKeys, 1 <= n_rows (<= max_rows unless that
// is 0), a dtype of the three, no NULL among the pointers the caller tested.  0, or DAAM_E_INVALID with the message set
int key_args_check(int n_keys, int dtype, int n_rows, int max_rows, bool null_arg);

}  // namespace daam
