// finalize_rect_kernel: compute_global_heat_map (reference daam/trace.py:103-126) for planes [h, w] and an output [out_h, out_w]
// of unequal sides -- the finalize of a non-square generation (daam_ctx_create_rect / daam_layer_configure_rect).
//
// Grid (token rows, key chunks [, groups]); workgroup (t, c) walks the keys c, c + n_chunks, ... of token t:
//   plane [h][w]  -- read from HBM once, in 16-byte pieces when the plane is a whole number of them (else element by element),
//                    widened to f32 into LDS
//   row pass      -- tmp[y][ox] = 4 border-clamped taps of bicubic_table(w, out_w) along the row          (LDS -> LDS)
//   column pass   -- v = 4 taps of bicubic_table(h, out_h) down the column of tmp; out tile += max(v, 0)   (LDS -> LDS)
// which is the order of torch's upsample_bicubic2d and of the general square kernel (daam_fin_kernel_body.inc); a key of the
// output's size is copy + clamp straight from HBM.  The workgroup's [out_h][out_w] tile lives in LDS across its keys and ends in
// one f32 atomic per element (x 1/N) into the zeroed output, as every finalize class kernel does.  f32 arithmetic throughout: the
// "any finite planes" accuracy class of include/daam_hip.h.  The host sizes the dynamic LDS (fin_rect_lds_bytes) and refuses a
// selection that needs more than a workgroup can have.
#include "daam_fin_rect.h"

namespace daam {

namespace {

// a plane element type: its 16-byte piece, and the element as f32
template <typename T> struct RectPlane;
template <> struct RectPlane<_Float16> {
    static constexpr int E = 8;
    using Piece = half8;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return (float)p[i]; }
    static __device__ __forceinline__ float one(const _Float16* s) { return (float)*as_global<_Float16>(s); }
};
template <> struct RectPlane<bf16_t> {
    static constexpr int E = 8;
    using Piece = ushort8;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return __uint_as_float((unsigned)p[i] << 16); }
    static __device__ __forceinline__ float one(const bf16_t* s) { return __uint_as_float((unsigned)*as_global<unsigned short>(s) << 16); }
};
template <> struct RectPlane<float> {
    static constexpr int E = 4;
    using Piece = float4v;
    static __device__ __forceinline__ float at(const Piece& p, int i) { return p[i]; }
    static __device__ __forceinline__ float one(const float* s) { return *as_global<float>(s); }
};

template <typename ACC_T>
__device__ __forceinline__ void finalize_rect_body(const FinRectLaunch& L)
{
    using P = RectPlane<ACC_T>;
    constexpr int E = P::E;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int tok = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int OH = L.out_h, OW = L.out_w, on = OH * OW;
    float* outt = reinterpret_cast<float*>(smem_raw);            // [OH][OW]
    float* plane = outt + ((on + 3) & ~3);                       // [h][w] of the current key (16-byte aligned)
    float* tmp = plane + L.plane_cap;                            // [h][OW]
    for (int i = tid; i < on; i += 256) outt[i] = 0.f;

    for (int kidx = chunk; kidx < L.n_keys; kidx += L.n_chunks) {
        const FinRectKey key = L.keys[kidx];
        const int h = key.h, w = key.w, n = h * w;
        const ACC_T* src = reinterpret_cast<const ACC_T*>(key.base) + (size_t)tok * n;
        const bool pieces = n % E == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;    // workgroup-uniform
        __syncthreads();                                         // the previous key is done with plane / tmp and with its share of outt
        if (key.tab < 0) {                                       // the output's size: copy + clamp (n == on)
            if (pieces) {
                for (int i = tid; i < n / E; i += 256) {
                    const typename P::Piece p = as_global<typename P::Piece>(src)[i];
#pragma unroll
                    for (int e = 0; e < E; ++e) outt[i * E + e] += fmaxf(P::at(p, e), 0.f);
                }
            } else {
                for (int i = tid; i < n; i += 256) outt[i] += fmaxf(P::one(src + i), 0.f);
            }
            continue;
        }
        const size_t tab_off = (size_t)key.tab * (OW + OH) * 4;
        const DAAM_GLOBAL int16_t* tix = as_global<int16_t>(L.tab_idx) + tab_off;   // row table, then the column table
        const DAAM_GLOBAL float* tw = as_global<float>(L.tab_w) + tab_off;
        if (pieces) {
            for (int i = tid; i < n / E; i += 256) {
                const typename P::Piece p = as_global<typename P::Piece>(src)[i];
#pragma unroll
                for (int e = 0; e < E; e += 4)
                    *reinterpret_cast<float4v*>(plane + i * E + e) = float4v{P::at(p, e), P::at(p, e + 1), P::at(p, e + 2), P::at(p, e + 3)};
            }
        } else {
            for (int i = tid; i < n; i += 256) plane[i] = P::one(src + i);
        }
        __syncthreads();
        for (int i = tid; i < h * OW; i += 256) {
            const int y = i / OW, ox = i - y * OW;
            const float* row = plane + y * w;
            const DAAM_GLOBAL int16_t* ix = tix + ox * 4;
            const DAAM_GLOBAL float* wt = tw + ox * 4;
            tmp[i] = row[ix[0]] * wt[0] + row[ix[1]] * wt[1] + row[ix[2]] * wt[2] + row[ix[3]] * wt[3];
        }
        __syncthreads();
        for (int i = tid; i < on; i += 256) {
            const int oy = i / OW, ox = i - oy * OW;
            const DAAM_GLOBAL int16_t* iy = tix + (OW + oy) * 4;
            const DAAM_GLOBAL float* wt = tw + (OW + oy) * 4;
            const float v = tmp[iy[0] * OW + ox] * wt[0] + tmp[iy[1] * OW + ox] * wt[1] +
                            tmp[iy[2] * OW + ox] * wt[2] + tmp[iy[3] * OW + ox] * wt[3];
            outt[i] += fmaxf(v, 0.f);
        }
    }
    __syncthreads();                                             // a copy key spreads outt over the threads in pieces: meet before the flush
    float* out = L.out + (size_t)tok * on;
    for (int i = tid; i < on; i += 256) atomicAdd(out + i, outt[i] * L.inv_n);
}

}  // namespace

template <typename ACC_T>
__global__ __launch_bounds__(256) void finalize_rect_kernel(const FinRectLaunch L)
{
    finalize_rect_body<ACC_T>(L);
}

// daam_finalize_groups: blockIdx.z = group; rows at or past the group's limit are neither read nor written
template <typename ACC_T>
__global__ __launch_bounds__(256) void finalize_rect_grouped_kernel(const FinRectGroupLaunch G)
{
    if ((int)blockIdx.x >= G.g[blockIdx.z].rows) return;
    finalize_rect_body<ACC_T>(fin_rect_group_view(G, blockIdx.z));
}

hipError_t launch_finalize_rect(const FinRectLaunch& L, const FinRectGroupLaunch* G, int n_groups, int tmp_cap, int dtype,
                                hipStream_t stream, int* grid_out, int* lds_out)
{
    const size_t lds = fin_rect_lds_bytes(L.out_h, L.out_w, L.plane_cap, tmp_cap);
    if (lds > kFinRectMaxLds) return hipErrorInvalidValue;     // (the caller has checked: never a launch that cannot fit)
    const dim3 grid(L.tokens, L.n_chunks, n_groups);
    *grid_out = fin_workgroups(grid);
    *lds_out = (int)lds;
    return fin_dispatch(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return G ? fin_launch(finalize_rect_grouped_kernel<T>, grid, 256, lds, stream, *G) : fin_launch(finalize_rect_kernel<T>, grid, 256, lds, stream, L);
    });
}

}  // namespace daam
