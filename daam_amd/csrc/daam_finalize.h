// The finalize (compute_global_heat_map, reference daam/trace.py:112-126) between its kernels (daam_finalize.hip,
// daam_finalize_pipe.hip, daam_finalize_rect.hip, daam_fin_bins.hip) and the host (daam_finalize_api.hip): the launch descriptors of
// the square class kernels, the device helpers more than one kernel file uses, the host's launch idiom (fin_dispatch: plane dtype
// -> element type; fin_launch: the one place a finalize kernel is launched) and the class launchers.  daam_fin_rect.h and
// daam_fin_bins.h add the descriptors and launchers of their kernels on top of this.
#pragma once
#include "daam_types.h"
#include "../../include/daam_hip.h"       // DAAM_F16 / DAAM_F32 / DAAM_BF16

namespace daam {

constexpr int kFinMaxChunks = 31;

// One selected (layer, head) key of a finalize launch.
struct FinKey {
    const void* base;       // plane of token 0: [tokens, side, side] follows
    int32_t side;
    int32_t tab;            // bicubic table index (-1: side == out_side, identity)
};

struct FinLaunch {
    const FinKey* keys;
    const int16_t* tab_idx; // [n_tabs][out_side][4] border-clamped tap indices
    const float* tab_w;     // [n_tabs][out_side][4] weights (A = -0.75)
    float* out;             // [tokens, out_side, out_side]
    int32_t n_keys;
    int32_t n_chunks;
    int32_t tokens;
    int32_t out_side;
    float inv_n;
    int32_t max_side;       // largest non-identity side among the keys (LDS carve-up)
    const void* mfma_ops;   // x2 MFMA finalize: [2 nt][64 lanes][6] 16-byte operand pieces (host-built), or NULL
    // x2 MFMA finalize: chunk c covers the keys [chunk_begin[c], chunk_begin[c + 1]) (even boundaries; its two key lanes take
    // them alternately); see finalize_chunk_ranges() in daam_finalize_api.hip.
    int16_t chunk_begin[kFinMaxChunks + 1];
};

// x2 finalize, software-pipelined kernel (daam_finalize_pipe.hip): workgroup (token, chunk) walks the plane pointers
// key_ptrs[chunk * ptr_stride + 0 .. nk_pad) (token 0's plane of each key, or the all-zero plane as padding; nk_pad even, >= 4,
// the same for every chunk; the ring prefetches kPipeRing + 1 entries past nk_pad, which must be valid pointers too).
struct FinPipeLaunch {
    const unsigned long long* key_ptrs;
    const unsigned long long* same_ptrs;   // [n_chunks][same_per] planes of token 0 of the 64 x 64 keys folded in (0 = padding), or NULL
    int32_t same_per;
    const void* mfma_ops;   // as FinLaunch::mfma_ops
    float* out;             // [tokens, 64, 64]
    int32_t n_chunks;
    int32_t nk_pad;
    int32_t ptr_stride;     // entries per chunk in key_ptrs
    int32_t tokens;
    float inv_n;
};

// daam_finalize_groups: one launch per class for N global heat maps.  blockIdx.z = group; the group fixes its key range
// (keys of one group are contiguous in the class's FinKey array / pointer tables), the row limit, 1/N and the output base.
// Workgroups with blockIdx.x past the group's rows exit at once (grid x is the largest row count).
constexpr int kFinMaxGroups = 64;
struct FinGroup {
    int32_t key_begin;      // first FinKey of the group in the class's array (general / same / up / x0.5 kernels)
    int32_t n_keys;
    int32_t rows;           // token rows of this group's output
    float inv_n;            // 1 / (keys of the group over every class)
    int64_t out_off;        // floats from FinLaunch::out / FinPipeLaunch::out to the group's [rows, O, O]
    int32_t ptr_off;        // pipelined x2 kernel: entries from key_ptrs / same_ptrs to the group's first chunk
    int32_t same_off;
};
struct FinGroupLaunch {
    FinLaunch L;            // shared fields; keys / n_keys / tokens / inv_n / out are per group
    FinGroup g[kFinMaxGroups];
};
struct FinPipeGroupLaunch {
    FinPipeLaunch L;
    FinGroup g[kFinMaxGroups];
};
// the group's view of a grouped launch
__host__ __device__ inline FinLaunch fin_group_view(const FinGroupLaunch& G, int g)
{
    FinLaunch L = G.L;
    L.keys += G.g[g].key_begin;
    L.n_keys = G.g[g].n_keys;
    L.tokens = G.g[g].rows;
    L.inv_n = G.g[g].inv_n;
    L.out += G.g[g].out_off;
    return L;
}

// ---- device helpers shared by the kernel files ---------------------------------------------------------------------------------
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

// max(a, b) for b >= 0 through the integer order of the bit patterns: one v_max_i32, no NaN canonicalisation in front
// (fmaxf() costs a second v_max_f32), and -- unlike an inline-asm v_max_f32 -- visible to the compiler's hazard
// recognizer, which pads the MFMA-result -> VALU-read wait states.  b >= 0: a negative a has its sign bit set and loses
// as an integer, two non-negative floats order like their bit patterns.
__device__ __forceinline__ float fin_max_nonneg(float a, float b) {
    const int x = __float_as_int(a), y = __float_as_int(b);
    return __int_as_float(x > y ? x : y);
}

// ---- the host's launch idiom ---------------------------------------------------------------------------------------------------
// fin_dispatch(dtype, fn): fn(tag) with the tag of the planes' dtype -- tag::type the element type a kernel is instantiated on,
// tag::dt the DAAM_* constant (the pipelined kernel's template argument).  F16: the spelling of fp16 in the kernel family; the
// general kernel (finalize_kernel) is instantiated on __half, everything else on _Float16.
template <typename T, int DT> struct FinType {
    using type = T;
    static constexpr int dt = DT;
};
template <typename F16 = _Float16, typename Fn> hipError_t fin_dispatch(int dtype, Fn&& fn)
{
    switch (dtype) {
    case DAAM_F16: return fn(FinType<F16, DAAM_F16>{});
    case DAAM_BF16: return fn(FinType<bf16_t, DAAM_BF16>{});
    case DAAM_F32: return fn(FinType<float, DAAM_F32>{});
    default: return hipErrorInvalidValue;
    }
}

// a kernel that wants more than the 64 KiB of dynamic LDS every kernel may have must be told so
template <typename K> hipError_t allow_lds(K kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <typename K, typename Arg>
hipError_t fin_launch(K kernel, dim3 grid, int block, size_t lds, hipStream_t stream, const Arg& arg)
{
    const hipError_t e = allow_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(block), lds, stream, arg);
    return hipGetLastError();
}
inline int fin_workgroups(dim3 grid) { return (int)(grid.x * grid.y * grid.z); }

// ---- class launchers ------------------------------------------------------------------------------------------------------------
// One per kernel family, for both of its forms: G == NULL launches the single-map kernel on L; otherwise L is G->L and the
// *_grouped_kernel runs on *G with grid z = n_groups (daam_finalize_groups).  dtype: DAAM_* of the planes.  grid_out / lds_out:
// workgroups and dynamic LDS bytes of the launch (lds_out is left alone by the kernels with static LDS).  FinClassLauncher is
// the signature the host's class table holds (daam_finalize_api.hip).
typedef hipError_t FinClassLauncher(const FinLaunch& L, const FinGroupLaunch* G, int n_groups, int dtype, hipStream_t stream,
                                    int* grid_out, int* lds_out);
FinClassLauncher launch_finalize;          // finalize_kernel: any side
FinClassLauncher launch_finalize_same;     // side == out_side
FinClassLauncher launch_finalize_down2;    // 128 -> 64
template <int S>                           // S = 32, 16 -> 64 (LDS kernel)
hipError_t launch_finalize_up(const FinLaunch& L, const FinGroupLaunch* G, int n_groups, int dtype, hipStream_t stream, int* grid_out,
                              int* lds_out);
bool finalize_up_supported(int side, int out_side);
bool finalize_down2_supported(int side, int out_side);
// x2 of fp16 planes on the matrix cores, round 2 (DAAM_NO_PIPE_FINALIZE=1): L.mfma_ops and L.chunk_begin set
hipError_t launch_finalize_up32_mfma(const FinLaunch& L, hipStream_t stream, int* grid_out);
// ... and both fp16 classes of an SDXL-1024 finalize in one launch (up: that kernel's class, same: the same-size class)
hipError_t launch_finalize_up32_same(const FinLaunch& up, const FinLaunch& same, hipStream_t stream, int* grid_out);
// x2 on the software-pipelined kernel; L.mfma_ops must be the operand set of `dtype` (bf16 planes: Wx in bf16)
hipError_t launch_finalize_up32_pipe(const FinPipeLaunch& L, const FinPipeGroupLaunch* G, int n_groups, int dtype,
                                     hipStream_t stream, int* grid_out);
int finalize_pipe_ring(int dtype);         // planes the ring prefetches past a chunk's last one (pointer-table padding)
// daam_finalize_groups: clear rows [0, rows[g]) of every group's output (out + g * stride floats), plane floats per row
hipError_t launch_zero_groups(float* out, size_t stride, int plane, const int* rows, int n_groups, hipStream_t stream);

}  // namespace daam
