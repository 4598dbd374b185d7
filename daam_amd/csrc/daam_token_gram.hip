// daam_token_gram (include/daam_analysis.h): per (layer, head) key the Gram matrix of its token planes, A * A^T on the matrix cores.
// token_gram_kernel<T, NB, WIDE>, grid n_keys x cap, 256 threads; workgroup (key, chunk of 1024 pixels), NB = blocks of 32 rows:
//   stage     -- a sub-tile [32 NB rows][128 px] (16-bit path) or [32 NB rows][64 px] f32 (WIDE: windows added as they arrive) goes
//                from HBM through registers into LDS, the next sub-tile's loads in flight while this one is multiplied; rows at or
//                past n_rows and pixels past the plane are zeros that never come from memory
//   multiply  -- a lane's fragment of row block b is 8 consecutive pixels of row 32 b + (lane & 31) (one f32 on the WIDE path): it is
//                the A operand of the blocks (b, *) and the B operand of the blocks (*, b).  Wave v takes a quarter of the sub-tile's
//                k-steps for all NB (NB + 1) / 2 blocks on and above the diagonal
//   join      -- block by block the four waves' accumulators meet in LDS, (w0 + w1) + (w2 + w3); the block is written once as it
//                is (lanes along a matrix row) and once mirrored (lanes along a matrix column, the same four values in the same
//                order), a diagonal block from its upper triangle alone: symmetric bit for bit, coalesced both times
// A one-chunk key writes gram[k] itself; the chunks of a longer key go to scratch and token_gram_join_kernel adds them in chunk order.
// No floating-point atomic.  The 16-bit path takes 16-byte pieces when the plane is a whole number of them from an aligned start
// (the rule of finalize_rect_kernel) and single elements otherwise; both fill the same LDS image, so the path does not show in the bits.
#include "daam_token_gram.h"

#include <cmath>

namespace daam {

namespace {

typedef __bf16 gram_bf16x8 __attribute__((ext_vector_type(8)));

template <typename T> __device__ __forceinline__ floatx16 gram_mfma16(const ushort8& a, const ushort8& b, const floatx16& c);
template <> __device__ __forceinline__ floatx16 gram_mfma16<_Float16>(const ushort8& a, const ushort8& b, const floatx16& c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ floatx16 gram_mfma16<bf16_t>(const ushort8& a, const ushort8& b, const floatx16& c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gram_bf16x8, a), __builtin_bit_cast(gram_bf16x8, b), c, 0, 0, 0);
}

constexpr int gram_lds_bytes(int nb, bool wide)
{
    const int stage = 32 * nb * (wide ? kGramRow32 * 4 : kGramRow16), join = 4 * kGramRed * 4;
    return stage > join ? stage : join;
}

}  // namespace

template <typename T, int NB, bool WIDE>
__global__ __launch_bounds__(kGramThreads) void token_gram_kernel(const GramLaunch L)
{
#pragma clang fp contract(off)
    constexpr int R = 32 * NB;                                   // staged rows
    constexpr int SUB = WIDE ? kGramSub32 : kGramSub16;
    constexpr int SLOTS = WIDE ? R * kGramSub32 / kGramThreads : R * (kGramSub16 / 8) / kGramThreads;     // 8 NB floats / 2 NB pieces
    constexpr int NT = NB * (NB + 1) / 2;
    __shared__ __align__(16) unsigned char smem[gram_lds_bytes(NB, WIDE)];
    float* const smem_f = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int k = blockIdx.x / L.cap, chunk = blockIdx.x - k * L.cap;
    const int n_rows = L.n_rows, rr = n_rows * n_rows;

    const DaamKeyPlanes key = L.keys[k];
    const bool ok = key_planes_ok(key);
    const int n = ok ? key.h * key.w : 0, n_chunks = gram_chunks(n), n_win = key.n_win;
    if (L.multi_only ? (!ok || n_win == 1) : (!WIDE && ok && n_win > 1)) return;        // the other launch's key
    if (!ok || n_chunks > L.cap) {                               // not a plane, or no room for its chunks: nothing is read
        if (chunk == 0)
            for (int i = tid; i < rr; i += kGramThreads) L.gram[(size_t)k * rr + i] = NAN;
        return;
    }
    if (chunk >= n_chunks) return;
    float* const dst = n_chunks == 1 ? L.gram + (size_t)k * rr : L.scratch + ((size_t)k * L.cap + chunk) * rr;
    const T* const base = reinterpret_cast<const T*>(key.base);
    const int64_t ws = key.win_stride;
    const int p0 = chunk * kGramChunk, pn = min(kGramChunk, n - p0), n_sub = (pn + SUB - 1) / SUB;

    floatx16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;

    if constexpr (WIDE) {
        float reg[SLOTS];
        // slot i = tid + 256 j: row i / 64, pixel i % 64 of the sub-tile (a wave reads 64 consecutive elements of one row)
        auto fetch = [&](int s) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int i = tid + kGramThreads * j, row = i >> 6, px = p0 + s * SUB + (i & 63);
                float v = 0.f;
                if (row < n_rows && px < n) {
                    const T* at = base + (size_t)row * n + px;
                    v = KeyElem<T>::one(at);
                    for (int wi = 1; wi < n_win; ++wi) v = v + KeyElem<T>::one(at + wi * ws);
                }
                reg[j] = v;
            }
        };
        fetch(0);
        for (int s = 0; s < n_sub; ++s) {
            __syncthreads();                                     // the last sub-tile's products are done with the image
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int i = tid + kGramThreads * j;
                smem_f[(i >> 6) * kGramRow32 + (i & 63)] = reg[j];
            }
            __syncthreads();
            if (s + 1 < n_sub) fetch(s + 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int at = 2 * (8 * wv + q) + (lane >> 5);
                float a[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) a[b] = smem_f[(32 * b + (lane & 31)) * kGramRow32 + at];
                int t = 0;
#pragma unroll
                for (int bi = 0; bi < NB; ++bi)
#pragma unroll
                    for (int bj = bi; bj < NB; ++bj, ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi], a[bj], acc[t], 0, 0, 0);
            }
        }
    } else {
        ushort8 reg[SLOTS];
        // 16-byte pieces: whole planes of them from an aligned start, so every row and every chunk starts on one (workgroup-uniform)
        const bool pieces = n % 8 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
        // slot i = tid + 256 j: row i / 16, piece i % 16 of the sub-tile (16 lanes read 256 consecutive bytes of one row)
        auto fetch = [&](int s) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int i = tid + kGramThreads * j, row = i >> 4, px = p0 + s * SUB + (i & 15) * 8;
                ushort8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (row < n_rows && px < n) {
                    const T* at = base + (size_t)row * n + px;
                    if (pieces) {
                        v = *as_global<ushort8>(at);
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (px + e < n) v[e] = as_global<unsigned short>(at)[e];
                    }
                }
                reg[j] = v;
            }
        };
        fetch(0);
        for (int s = 0; s < n_sub; ++s) {
            __syncthreads();                                     // the last sub-tile's products are done with the image
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int i = tid + kGramThreads * j;
                *reinterpret_cast<ushort8*>(smem + (i >> 4) * kGramRow16 + (i & 15) * 16) = reg[j];
            }
            __syncthreads();
            if (s + 1 < n_sub) fetch(s + 1);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int at = (16 * (2 * wv + q) + 8 * (lane >> 5)) * 2;
                ushort8 a[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) a[b] = *reinterpret_cast<const ushort8*>(smem + (32 * b + (lane & 31)) * kGramRow16 + at);
                int t = 0;
#pragma unroll
                for (int bi = 0; bi < NB; ++bi)
#pragma unroll
                    for (int bj = bi; bj < NB; ++bj, ++t) acc[t] = gram_mfma16<T>(a[bi], a[bj], acc[t]);
            }
        }
    }

    // join: C/D element of register g, lane l is (row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31) of the block
    int t = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
#pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++t) {
            __syncthreads();                                     // the image, or the last block, has been read
#pragma unroll
            for (int g = 0; g < 16; ++g) smem_f[wv * kGramRed + g * 65 + lane] = acc[t][g];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = tid + kGramThreads * q;
                {                                                // as it is: lanes along the block's columns
                    const int g = e >> 6, l = e & 63, at = g * 65 + l;
                    const int i = 32 * bi + (g & 3) + 8 * (g >> 2) + 4 * (l >> 5), j = 32 * bj + (l & 31);
                    const float v = (smem_f[at] + smem_f[kGramRed + at]) + (smem_f[2 * kGramRed + at] + smem_f[3 * kGramRed + at]);
                    if (i < n_rows && j < n_rows && (bi != bj || i <= j)) dst[i * n_rows + j] = v;
                }
                {                                                // mirrored: lanes along the block's rows
                    const int r = e & 31, c = e >> 5, g = (r & 3) + 4 * (r >> 3), l = 32 * ((r >> 2) & 1) + c, at = g * 65 + l;
                    const int i = 32 * bi + r, j = 32 * bj + c;
                    const float v = (smem_f[at] + smem_f[kGramRed + at]) + (smem_f[2 * kGramRed + at] + smem_f[3 * kGramRed + at]);
                    if (i < n_rows && j < n_rows && (bi != bj || i < j)) dst[j * n_rows + i] = v;
                }
            }
        }
    }
}

// gram[k] = the key's chunk matrices added in chunk order; grid n_keys.  One-chunk keys and keys that are NaN are already written.
__global__ __launch_bounds__(kGramThreads) void token_gram_join_kernel(const GramLaunch L)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x, rr = L.n_rows * L.n_rows;
    const DaamKeyPlanes key = L.keys[k];
    if (!key_planes_ok(key)) return;
    const int n_chunks = gram_chunks(key.h * key.w);
    if (n_chunks == 1 || n_chunks > L.cap) return;
    const float* part = L.scratch + (size_t)k * L.cap * rr;
    for (int i = threadIdx.x; i < rr; i += kGramThreads) {
        float v = part[i];
        for (int c = 1; c < n_chunks; ++c) v = v + part[(size_t)c * rr + i];
        L.gram[(size_t)k * rr + i] = v;
    }
}

namespace {

template <typename T, bool WIDE> hipError_t gram_launch_nb(int nb, dim3 grid, hipStream_t stream, const GramLaunch& L)
{
    switch (nb) {
    case 1: return fin_launch(token_gram_kernel<T, 1, WIDE>, grid, kGramThreads, 0, stream, L);
    case 2: return fin_launch(token_gram_kernel<T, 2, WIDE>, grid, kGramThreads, 0, stream, L);
    default: return fin_launch(token_gram_kernel<T, 3, WIDE>, grid, kGramThreads, 0, stream, L);
    }
}

bool gram_sizes_ok(int n_keys, int n_rows) { return n_keys >= 1 && n_keys <= kKeyMaxKeys && n_rows >= 1 && n_rows <= kGramMaxRows; }

}  // namespace

}  // namespace daam

using namespace daam;

size_t daam_token_gram_scratch_bytes(int n_keys, int n_rows, int max_hw)
{
    if (!gram_sizes_ok(n_keys, n_rows) || max_hw < 1) return 0;
    const int hw = max_hw < kKeyMaxSide * kKeyMaxSide ? max_hw : kKeyMaxSide * kKeyMaxSide;
    return (size_t)n_keys * gram_chunks(hw) * n_rows * n_rows * sizeof(float);
}

int daam_token_gram(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, float* gram, void* scratch, size_t scratch_bytes,
                    void* stream)
{
    if (key_args_check(n_keys, dtype, n_rows, kGramMaxRows, !keys || !gram || !scratch)) return DAAM_E_INVALID;
    const size_t per_chunk = (size_t)n_keys * n_rows * n_rows * sizeof(float);
    if (scratch_bytes < per_chunk)
        return analysis_fail(DAAM_E_INVALID, "scratch of %zu bytes: %d keys of %d rows need %zu per chunk of %d pixels", scratch_bytes, n_keys,
                         n_rows, per_chunk, kGramChunk);

    GramLaunch L;
    L.keys = keys; L.gram = gram; L.scratch = static_cast<float*>(scratch);
    L.n_keys = n_keys; L.n_rows = n_rows;
    const size_t cap = scratch_bytes / per_chunk;
    L.cap = (int32_t)(cap < (size_t)kGramMaxChunks ? cap : (size_t)kGramMaxChunks);
    L.multi_only = 0;
    const int nb = (n_rows + 31) / 32;
    const dim3 grid((unsigned)((int64_t)n_keys * L.cap));
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (dtype != DAAM_F32) {                                     // the 16-bit path takes the keys of one window (and the NaN keys)
        e = fin_dispatch(dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            if constexpr (sizeof(T) == 2) return gram_launch_nb<T, false>(nb, grid, s, L);
            else return hipErrorInvalidValue;
        });
        L.multi_only = 1;
    }
    if (e == hipSuccess)
        e = fin_dispatch(dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            return gram_launch_nb<T, true>(nb, grid, s, L);
        });
    if (e == hipSuccess && L.cap > 1) e = fin_launch(token_gram_join_kernel, dim3((unsigned)n_keys), kGramThreads, 0, s, L);
    if (e != hipSuccess) return analysis_fail((int)e, "token gram: %s", hipGetErrorString(e));
    return 0;
}
