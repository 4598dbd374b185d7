// Element helpers of the any-dtype kernels (the generic and the probs tap in daam_kernels.hip, the general finalize kernel in
// daam_finalize.hip): load / store an element as f32, and "round_to<T>", which reproduces the rounding point of a tensor that the
// reference pipeline materialises in dtype T (fp16 logits / probabilities), returning the value as f32.
#pragma once
#include "daam_types.h"

namespace daam {

template <typename T> __device__ __forceinline__ float ld(const T* p);
template <> __device__ __forceinline__ float ld<__half>(const __half* p) { return __half2float(*p); }
template <> __device__ __forceinline__ float ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }

template <typename T> __device__ __forceinline__ float round_to(float x);
template <> __device__ __forceinline__ float round_to<__half>(float x) { return __half2float(__float2half_rn(x)); }
template <> __device__ __forceinline__ float round_to<float>(float x) { return x; }
template <> __device__ __forceinline__ float round_to<bf16_t>(float x) { return bf16_to_f32(f32_to_bf16(x)); }

// acc = acc + x in the accumulator dtype.  For fp16 the f32 add of two fp16 values followed by
// one RNE rounding is the correctly rounded fp16 add (24 >= 2*11+2 bits), i.e. exactly what
// torch's / numpy's half add does (heatmap.py:156).
template <typename T> __device__ __forceinline__ void st(T* p, float v);
template <> __device__ __forceinline__ void st<__half>(__half* p, float v) { *p = __float2half_rn(v); }
template <> __device__ __forceinline__ void st<float>(float* p, float v) { *p = v; }
// bf16: f32 add of two bf16 values + one RNE rounding = the correctly rounded bf16 add (24 >= 2*8+2 bits)
template <> __device__ __forceinline__ void st<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }

}  // namespace daam
