// Device text shared by the epilogue kernels: the word-map kernels and the pair overlap (daam_epilogue.hip), the batched word masks
// (daam_word_masks.hip), the overlap matrix (daam_mask_matrix.hip) and the region scores (daam_region_scores.hip).  Everything here
// is force-inlined, and a piece lives here only where the machine code of every kernel that uses it stayed byte for byte what it was
// with the text written out in place (profiles/epilogue_refactor.json lists what was tried, DESIGN 3.14 what stayed behind).
#pragma once
#include "daam_types.h"

namespace daam {

// Keys' cubic convolution weights (A = -0.75) of the four taps around a source coordinate with fraction t, in the operation order of
// torch's upsample_bicubic2d, every product and sum rounded on its own (contraction off).  The float64 oracles count the roundings
// of exactly this order: tests/_epilogue_domain.py (`cubic_weights`, `horner_error`) and tests/_region_domain.py (`roundings`).
// A change of the order is a change of those files.
__device__ __forceinline__ void cubic_coeffs(float t, float w[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float x0 = t + 1.0f;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    const float u = 1.0f - t;
    w[2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
    const float x3 = u + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

// Output index o of an axis resized by scale = n_in / n_out (align_corners=False): the weights of its four taps; returns the source
// index of the first one.  The caller clamps first .. first + 3 to its border: with the clamp loop in here too, the expand kernels,
// mask_overlap_kernel and region_tables_kernel came out as other machine code (profiles/epilogue_refactor.json).
__device__ __forceinline__ int cubic_taps(float scale, int o, float w[4]) {
#pragma clang fp contract(off)
    const float src = scale * ((float)o + 0.5f) - 0.5f;
    const float f = floorf(src);
    cubic_coeffs(src - f, w);
    return (int)f - 1;
}

// The x pass of the 4 x 4 gather on one source row r; the callers run it on their four rows and then combine those with the y
// weights in the same way (the order of torch's upsample_bicubic2d).
__device__ __forceinline__ float cubic_row(const float* r, const int ix[4], const float wx[4]) {
#pragma clang fp contract(off)
    return r[ix[0]] * wx[0] + r[ix[1]] * wx[1] + r[ix[2]] * wx[2] + r[ix[3]] * wx[3];
}

// Order-preserving int encoding of a float: a < b as floats <=> enc(a) < enc(b) as ints, so atomicMin / atomicMax on ints give a
// float min / max.  kEncPosInf / kEncNegInf start such a pair.
__device__ __forceinline__ int enc_ordered(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float dec_ordered(int i) {
    return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff);
}
constexpr int kEncPosInf = 0x7f800000;                                     // enc_ordered(+inf)
constexpr int kEncNegInf = (int)0x80000000 ^ 0x7fffffff ^ 0x7f800000;      // enc_ordered(-inf)

// Results the caller copies to the host right behind the kernel (expand_as returns a CPU tensor, heatmap.py:88) are stored write-through
// (system scope): the copy engine reads memory, not the L2s.  Round 6 saw ONE expand_as result in ~10^5 whose 64 consecutive elements (two
// cache lines) still held the block's previous owner's data after the copy (four test processes sharing the GPU; not reproduced in 80 000
// calls) -- with write-through stores the result does not depend on when an L2 writes a dirty line back.
__device__ __forceinline__ void store_for_host(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// u8 mask bytes -> bit sets.  bit b of the result = byte b of the 16 is not zero.  Per dword: bit 7 of every byte = "byte != 0" (the
// carry out of the low seven bits, or the byte's own bit 7), then one dot product with the weights 1, 2, 4, ... gathers the four of them.
__device__ __forceinline__ uint32_t mask_nonzero(uint32_t x)
{
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}
__device__ __forceinline__ uint32_t mask_bits16(uint4 v)
{
    uint32_t lo = __builtin_amdgcn_udot4(mask_nonzero(v.x), 0x08040201u, 0u, false);
    lo = __builtin_amdgcn_udot4(mask_nonzero(v.y), 0x80402010u, lo, false);
    uint32_t hi = __builtin_amdgcn_udot4(mask_nonzero(v.z), 0x08040201u, 0u, false);
    hi = __builtin_amdgcn_udot4(mask_nonzero(v.w), 0x80402010u, hi, false);
    return (lo >> 7) | (hi << 1);              // the sums are 128 x (8 bits)
}

// the same for a chunk that reaches outside [lo, hi): bytes outside count as zero and are not read
__device__ __forceinline__ uint32_t mask_bits16_edge(const uint8_t* p, const uint8_t* lo, const uint8_t* hi)
{
    uint32_t bits = 0;
#pragma unroll 1
    for (int b = 0; b < 16; ++b)
        if (p + b >= lo && p + b < hi && p[b] != 0) bits |= 1u << b;
    return bits;
}

}  // namespace daam
