// Window-range reduction of daam_finalize_bins (time-binned context): for every (group, selected key) task, the planes
// of the windows [bin_begin, bin_end) are added in window order, in f32, into an f32 scratch plane set.  The existing
// finalize classes then run on the scratch planes: the clamp of the reference (daam/trace.py:118-124) is not linear, so
// the windows' sums must be added BEFORE the bicubic, exactly as the running sum of a generation that ran only those
// steps would hold them (daam/heatmap.py:153-156 adds step after step into one tensor).
//
// One launch for every task of the call; workgroup = 256 threads x one 16-byte load per window per thread (8 fp16 /
// bf16 or 4 f32 elements).  The workgroup finds its task by a binary search over tile_begin (uniform across the
// workgroup).  Rows the caller crops away are outside [0, n_elem): neither read nor written.
#include "daam_fin_bins.h"

namespace daam {

typedef unsigned bin_u32x4 __attribute__((ext_vector_type(4)));
typedef float bin_f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct BinVec;
template <> struct BinVec<_Float16> {
    static constexpr int V = 8;
    __device__ static float at(const _Float16* p, int i) { return (float)p[i]; }
};
template <> struct BinVec<bf16_t> {
    static constexpr int V = 8;
    __device__ static float at(const bf16_t* p, int i) { return bf16_to_f32(p[i]); }
};
template <> struct BinVec<float> {
    static constexpr int V = 4;
    __device__ static float at(const float* p, int i) { return p[i]; }
};

template <typename T>
__global__ __launch_bounds__(kBinSumThreads) void finalize_bin_sum_kernel(BinSumLaunch L)
{
    constexpr int V = BinVec<T>::V;
    const int tile = blockIdx.x;
    int lo = 0, hi = L.n_tasks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L.tasks[mid].tile_begin <= tile) lo = mid;
        else hi = mid - 1;
    }
    const BinSumTask t = L.tasks[lo];
    const int64_t e0 = ((int64_t)(tile - t.tile_begin) * kBinSumThreads + threadIdx.x) * V;
    if (e0 >= t.n_elem) return;
    const T* src = static_cast<const T*>(t.src);
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    if (t.vec && e0 + V <= t.n_elem) {
        for (int w = 0; w < t.n_win; ++w) {
            const bin_u32x4 raw = *as_global<bin_u32x4>(src + (int64_t)w * t.win_stride + e0);
            const T* v = reinterpret_cast<const T*>(&raw);
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] += BinVec<T>::at(v, i);
        }
        DAAM_GLOBAL bin_f32x4* d = as_global_rw<bin_f32x4>(t.dst + e0);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) d[i] = bin_f32x4{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
        return;
    }
    // unaligned planes or the tail of an odd-sized task: element by element
    const int n = (int)((t.n_elem - e0) < V ? (t.n_elem - e0) : V);
    for (int w = 0; w < t.n_win; ++w)
        for (int i = 0; i < n; ++i) acc[i] += BinVec<T>::at(src + (int64_t)w * t.win_stride + e0, i);
    for (int i = 0; i < n; ++i) t.dst[e0 + i] = acc[i];
}

int bin_sum_elems_per_tile(int dtype) { return kBinSumThreads * (dtype == DAAM_F32 ? BinVec<float>::V : BinVec<_Float16>::V); }

hipError_t launch_finalize_bin_sum(const BinSumLaunch& L, int dtype, hipStream_t stream)
{
    if (L.n_tasks <= 0 || L.n_tiles <= 0) return hipSuccess;
    return fin_dispatch(dtype, [&](auto t) {
        return fin_launch(finalize_bin_sum_kernel<typename decltype(t)::type>, dim3(L.n_tiles), kBinSumThreads, 0, stream, L);
    });
}

}  // namespace daam
