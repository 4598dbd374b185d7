// What every specialised tap kernel asks of a call's addressing, written once for their tap_*_supported() predicates
// (host only; the kernel files include it behind their kernels).
#pragma once
#include "../../include/daam_hip.h"

#include <stdint.h>

namespace daam {

// Q / K rows are fetched and the running sums updated in 16-byte pieces (8 fp16 / bf16 elements): hw and every stride a multiple of
// 8 elements, both pointers 16-byte aligned.  non_negative: the kernel also needs every stride >= 0 (chunk, slab; the others leave
// that to offsets_fit_32() in daam_tap_api.hip).
inline bool tap_rows_16b(const DaamQKDesc& d, const void* q, const void* k, bool non_negative)
{
    if (d.hw % 8 != 0) return false;
    const int64_t s[] = {d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h, d.k_stride_b, d.k_stride_h};
    for (int64_t v : s)
        if (v % 8 != 0 || (non_negative && v < 0)) return false;
    return ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0;
}

}  // namespace daam
