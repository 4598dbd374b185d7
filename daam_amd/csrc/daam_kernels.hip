// Baseline (any head_dim, any dtype combo) tap kernels of the DAAM heat-map extraction path for
// gfx950, and the launches' plumbing.  The fp16 MFMA tap lives in daam_tap_mfma.hip; this file holds
//   * tap_generic_kernel   : softmax(scale q k^T) -> conditional half -> running sums
//                            (reference daam/trace.py:276-294 + daam/heatmap.py:153-156)
//   * tap_probs_kernel     : the same accumulate from materialised probabilities
//   * upload_kernel (the tap's and the finalize's device tables), clock_monitor_kernel, start_gate_kernel
// (every finalize kernel: daam_finalize*.hip, daam_fin_bins.hip; normalise, word maps and the pair overlap: daam_epilogue.hip)
#include "daam_elem.h"

namespace daam {

// XCD-aware block remap: hardware places block b on XCD b % 8; give each XCD a contiguous
// range of logical tiles so the tiles of one (layer, head) - which share K - share an L2.
__device__ __forceinline__ int logical_block(int total_wgs, int wgs_per_xcd) {
    const int b = blockIdx.x;
    const int l = (b & 7) * wgs_per_xcd + (b >> 3);
    return l < total_wgs ? l : -1;
}

__device__ __forceinline__ int find_layer(const TapLayer* layers, int n, int wg) {
    int lo = 0, hi = n - 1;                       // last layer with wg_begin <= wg
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (layers[mid].wg_begin <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------
// Generic tap.  256 threads = 64 pixels x 4 token chunks.  Thread (p, part) owns the running
// sums acc[t][p0 + p] for its <= 20 tokens in registers across every step of the launch.
// LDS: K of the current (step, head) as f32 [tokens][d] (broadcast reads), plus the
// cross-chunk softmax reductions.
// ---------------------------------------------------------------------------------------
template <typename IN_T, typename ACC_T>
__global__ __launch_bounds__(256) void tap_generic_kernel(const TapLaunch L)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wg = logical_block(L.total_wgs, L.wgs_per_xcd);
    if (wg < 0) return;

    TapLayer lay;
    const TapPtr* ptrs;
    if (L.layers) {
        lay = L.layers[find_layer(L.layers, L.n_layers, wg)];
        ptrs = L.ptrs + lay.ptr_begin;
    } else {
        lay = L.one;
        ptrs = &L.one_ptr;
    }
    const int tokens = L.tokens;
    const int d = lay.head_dim;
    const int rel = wg - lay.wg_begin;
    const int kh = rel / lay.tiles_per_head;              // kept-head index 0..heads_kept-1
    const int p0 = (rel - kh * lay.tiles_per_head) * kTapPixels;
    const int bh = lay.bh_first + kh;
    const int b = bh / lay.heads, h = bh - b * lay.heads;

    float* Ks = reinterpret_cast<float*>(smem_raw);        // [tokens][d]
    float* red = Ks + tokens * d;                          // [2][kTapParts][kTapPixels]

    const int tid = threadIdx.x;
    const int p = tid & (kTapPixels - 1);
    const int part = tid >> 6;
    const int pixel = p0 + p;
    const bool valid = pixel < lay.hw;
    const int t0 = part * kTokPerPart;
    const int nt = min(kTokPerPart, tokens - t0);          // may be <= 0 for tiny token counts

    ACC_T* acc = reinterpret_cast<ACC_T*>(lay.acc) + (size_t)kh * tokens * lay.hw;
    float run[kTokPerPart];
#pragma unroll
    for (int i = 0; i < kTokPerPart; ++i)
        run[i] = (valid && i < nt) ? ld<ACC_T>(acc + (size_t)(t0 + i) * lay.hw + pixel) : 0.f;

    for (int s = 0; s < lay.n_steps; ++s) {
        const IN_T* q = reinterpret_cast<const IN_T*>(ptrs[s].q) + b * lay.q_sb + h * lay.q_sh;
        const IN_T* k = reinterpret_cast<const IN_T*>(ptrs[s].k) + b * lay.k_sb + h * lay.k_sh;
        __syncthreads();                                   // previous step done with Ks / red
        for (int i = tid; i < tokens * d; i += 256) {
            const int t = i / d, dd = i - t * d;
            Ks[i] = ld<IN_T>(k + t * lay.k_st + dd);
        }
        __syncthreads();

        float logit[kTokPerPart];
#pragma unroll
        for (int i = 0; i < kTokPerPart; ++i) logit[i] = 0.f;
        if (valid) {
            const IN_T* qrow = q + (int64_t)pixel * lay.q_sp;
            for (int dd = 0; dd < d; ++dd) {
                const float qv = ld<IN_T>(qrow + dd);
#pragma unroll
                for (int i = 0; i < kTokPerPart; ++i)
                    if (i < nt) logit[i] = fmaf(qv, Ks[(t0 + i) * d + dd], logit[i]);
            }
        }
        // alpha applied in f32 to the f32 dot product, then the baddbmm output rounding
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < kTokPerPart; ++i) {
            float x = logit[i] * lay.scale;
            if (lay.round_logits) x = round_to<IN_T>(x);
            logit[i] = x;
            if (i < nt) m = fmaxf(m, x);
        }
        red[part * kTapPixels + p] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[p], red[kTapPixels + p]), fmaxf(red[2 * kTapPixels + p], red[3 * kTapPixels + p]));
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < kTokPerPart; ++i) {
            const float e = (i < nt) ? expf(logit[i] - m) : 0.f;
            logit[i] = e;
            sum += e;
        }
        float* rsum = red + kTapParts * kTapPixels;
        rsum[part * kTapPixels + p] = sum;
        __syncthreads();
        sum = (rsum[p] + rsum[kTapPixels + p]) + (rsum[2 * kTapPixels + p] + rsum[3 * kTapPixels + p]);
#pragma unroll
        for (int i = 0; i < kTokPerPart; ++i) {
            const float prob = round_to<IN_T>(logit[i] / sum);       // probs.to(dtype)
            run[i] = round_to<ACC_T>(run[i] + prob);                  // heatmap.py:156
        }
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < kTokPerPart; ++i)
            if (i < nt) st<ACC_T>(acc + (size_t)(t0 + i) * lay.hw + pixel, run[i]);
    }
}

// ---------------------------------------------------------------------------------------
// Tap from materialised probabilities [BH, hw, tokens] (contiguous).  The 64-pixel chunk of
// one head is one contiguous run of 64*tokens elements: stage it through LDS with coalesced
// reads, then the same (pixel, token-chunk) ownership as above does the transposed add.
// ---------------------------------------------------------------------------------------
template <typename IN_T, typename ACC_T>
__global__ __launch_bounds__(256) void tap_probs_kernel(const ProbsLaunch L)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wg = logical_block(L.total_wgs, L.wgs_per_xcd);
    if (wg < 0) return;
    const int tokens = L.tokens;
    const int kh = wg / L.tiles_per_head;
    const int p0 = (wg - kh * L.tiles_per_head) * kTapPixels;
    const int npix = min(kTapPixels, L.hw - p0);
    IN_T* raw = reinterpret_cast<IN_T*>(smem_raw);         // [npix][tokens]
    const IN_T* src = reinterpret_cast<const IN_T*>(L.probs) + ((size_t)(L.bh_first + kh) * L.hw + p0) * tokens;
    const int tid = threadIdx.x;
    const int n = npix * tokens;
    for (int i = tid; i < n; i += 256) raw[i] = src[i];
    __syncthreads();
    const int p = tid & (kTapPixels - 1);
    const int part = tid >> 6;
    if (p >= npix) return;
    const int t0 = part * kTokPerPart;
    const int nt = min(kTokPerPart, tokens - t0);
    ACC_T* acc = reinterpret_cast<ACC_T*>(L.acc) + (size_t)kh * tokens * L.hw + (p0 + p);
    for (int i = 0; i < nt; ++i) {
        ACC_T* a = acc + (size_t)(t0 + i) * L.hw;
        st<ACC_T>(a, ld<ACC_T>(a) + ld<IN_T>(raw + p * tokens + t0 + i));
    }
}

// per-launch device tables: pinned host (device-mapped) -> device twin, in stream order on the
// compute queue (16 bytes per thread; tables are a few tens of KB)
__global__ __launch_bounds__(256) void upload_kernel(float4* dst, const float4* src, int n16, float4* zero, int z16)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
    else if (i - n16 < z16) zero[i - n16] = float4{0.f, 0.f, 0.f, 0.f};
}

// `zero` / `zero_bytes` (16-byte multiple, may be 0): a buffer cleared by the same launch (the finalize
// output, which is accumulated with atomics) -- saves a separate memset on the critical path
hipError_t launch_upload(void* dst, const void* src_host_mapped, size_t bytes, void* zero, size_t zero_bytes,
                         hipStream_t stream)
{
    const int n16 = (int)((bytes + 15) / 16);                 // ring slots are 256-byte aligned and padded
    const int z16 = (int)(zero_bytes / 16);
    hipLaunchKernelGGL(upload_kernel, dim3((n16 + z16 + 255) / 256), dim3(256), 0, stream, reinterpret_cast<float4*>(dst),
                       reinterpret_cast<const float4*>(src_host_mapped), n16, reinterpret_cast<float4*>(zero), z16);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// host-callable launchers (called from daam_api.hip / daam_tap_api.hip)
// ---------------------------------------------------------------------------------------
hipError_t launch_tap_generic(const TapLaunch& L, int in_dtype, int acc_dtype, int max_d, hipStream_t stream,
                              int* grid_out, int* lds_out)
{
    const size_t lds = (size_t)L.tokens * max_d * sizeof(float) + 2 * kTapParts * kTapPixels * sizeof(float);
    const int grid = L.wgs_per_xcd * 8;
    *grid_out = grid;
    *lds_out = (int)lds;
    hipError_t e;
#define DAAM_LAUNCH(IN, ACC)                                                            \
    do {                                                                                \
        if (lds > 64 * 1024 &&                                                          \
            (e = hipFuncSetAttribute(reinterpret_cast<const void*>(tap_generic_kernel<IN, ACC>),                     \
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e; \
        hipLaunchKernelGGL((tap_generic_kernel<IN, ACC>), dim3(grid), dim3(256), lds, stream, L); \
    } while (0)
    if (in_dtype == 0 && acc_dtype == 0) DAAM_LAUNCH(__half, __half);
    else if (in_dtype == 0 && acc_dtype == 1) DAAM_LAUNCH(__half, float);
    else if (in_dtype == 2 && acc_dtype == 2) DAAM_LAUNCH(bf16_t, bf16_t);
    else if (in_dtype == 2 && acc_dtype == 1) DAAM_LAUNCH(bf16_t, float);
    else if (in_dtype == 1 && acc_dtype == 1) DAAM_LAUNCH(float, float);
    else return hipErrorInvalidValue;
#undef DAAM_LAUNCH
    return hipGetLastError();
}

hipError_t launch_tap_probs(const ProbsLaunch& L, int in_dtype, int acc_dtype, hipStream_t stream, int* grid_out,
                            int* lds_out)
{
    const size_t lds = (size_t)kTapPixels * L.tokens * (in_dtype == 1 ? 4 : 2);
    const int grid = L.wgs_per_xcd * 8;
    *grid_out = grid;
    *lds_out = (int)lds;
    if (in_dtype == 0 && acc_dtype == 0)
        hipLaunchKernelGGL((tap_probs_kernel<__half, __half>), dim3(grid), dim3(256), lds, stream, L);
    else if (in_dtype == 0 && acc_dtype == 1)
        hipLaunchKernelGGL((tap_probs_kernel<__half, float>), dim3(grid), dim3(256), lds, stream, L);
    else if (in_dtype == 2 && acc_dtype == 2)
        hipLaunchKernelGGL((tap_probs_kernel<bf16_t, bf16_t>), dim3(grid), dim3(256), lds, stream, L);
    else if (in_dtype == 2 && acc_dtype == 1)
        hipLaunchKernelGGL((tap_probs_kernel<bf16_t, float>), dim3(grid), dim3(256), lds, stream, L);
    else if (in_dtype == 1 && acc_dtype == 1)
        hipLaunchKernelGGL((tap_probs_kernel<float, float>), dim3(grid), dim3(256), lds, stream, L);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// Shader-clock monitor (daam_clock_monitor_start): ONE wave; lane 0 stores (shader cycles, 100 MHz reference ticks) every
// `period_us`, sleeping in between (s_sleep keeps it off the issue ports of the kernels under test).
__global__ __launch_bounds__(64) void clock_monitor_kernel(unsigned long long* samples, int n_samples, int period_us)
{
    if (threadIdx.x != 0) return;
    const unsigned long long period = (unsigned long long)period_us * 100ull;       // reference ticks
    unsigned long long next = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < n_samples; ++i) {
        while (__builtin_amdgcn_s_memrealtime() < next) __builtin_amdgcn_s_sleep(32);
        const unsigned long long cyc = __builtin_amdgcn_s_memtime();
        const unsigned long long ref = __builtin_amdgcn_s_memrealtime();
        __hip_atomic_store(samples + 2 * i, cyc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(samples + 2 * i + 1, ref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        next = ref + period;
    }
}

hipError_t launch_clock_monitor(unsigned long long* samples, int n_samples, int period_us, hipStream_t stream)
{
    hipLaunchKernelGGL(clock_monitor_kernel, dim3(1), dim3(64), 0, stream, samples, n_samples, period_us);
    return hipGetLastError();
}

// Start gate of a multi-kernel tap flush (SD-v1.5: head_dim 40 / 80 / 160 = three kernels).  The small kernels run on side
// streams behind an event wait, the large one on the caller's stream -- and when the large one's 1024 workgroups are dispatched
// first they take every CU's LDS for their whole 50-step life and the small kernels only start when they drain (measured: 495 us
// per flush against 435 us when the small kernels' workgroups are resident first and the large grid fills in around them).  One
// wave on the caller's stream, ahead of the large kernel: wait until the side kernels' workgroups have counted themselves in
// (TapLaunch::started), or for `timeout_us` -- it holds no LDS and one wave slot, so it can never keep them from starting.
// A gate that runs into its timeout (the auxiliary streams did NOT run beside the caller's: e.g. mapped onto one hardware queue)
// says so in `timeouts` (pinned host memory, device-mapped): the host then stops using the gate for the context.
__global__ __launch_bounds__(64) void start_gate_kernel(const unsigned* counter, unsigned target, int timeout_us, unsigned* timeouts)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();                 // 100 MHz
    const unsigned long long limit = (unsigned long long)timeout_us * 100ull;
    while ((int)(__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit) {
            if (timeouts && threadIdx.x == 0) __hip_atomic_fetch_add(timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(4);
    }
}

hipError_t launch_start_gate(const unsigned* counter, unsigned target, int timeout_us, unsigned* timeouts, hipStream_t stream)
{
    hipLaunchKernelGGL(start_gate_kernel, dim3(1), dim3(64), 0, stream, counter, target, timeout_us, timeouts);
    return hipGetLastError();
}

}  // namespace daam
