// daam_key_scores (include/daam_analysis.h): per (layer, head) key and token row, the clamped bicubic resize of the running sum
// weighed by up to 32 region footprints -- the finalize's arithmetic per key with a dot product where the finalize has its sum
// over keys.  key_scores_kernel, grid n_keys x n_chunks, 256 threads; workgroup (key, chunk of token rows):
//   tap tables    -- index + 4 weights per output column and per output row (cubic_taps of daam_epilogue.h), once, in LDS
//   per batch of <= 4 token rows:
//     planes      -- read from HBM once, in 16-byte pieces when the plane is a whole number of them and the address allows (else
//                    element by element), the windows added in f32 as they arrive, into the row's own tile
//     row pass    -- tmp[y][ox] = 4 taps along the row                                                    (LDS -> LDS)
//     column pass -- tile[oy][ox] = max(4 taps down the column of tmp, 0), over the plane it came from    (LDS -> LDS)
//     dots        -- four footprints at a time: a lane reads each footprint element once for the batch and each tile element once
//                    for the four footprints; 16 chains per lane, a butterfly per wave, the four waves in order
// A key of the output's size is loaded and clamped straight into its tile.  A key whose plane or row pass does not fit the
// staging (a down-sampling key: more cells than the output) gathers its 16 taps per output element from global memory instead, in
// the same operation order, so the path taken does not show in the bits.  No floating-point atomic; every product and sum of the
// resize is rounded on its own (contraction off), the dots are explicit fused multiply-adds.
#include "daam_key_scores.h"
#include "daam_epilogue.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

namespace {

// element i of a token row's plane: the windows added in window order
template <typename T> __device__ __forceinline__ float ks_elem(const T* row, int64_t win_stride, int n_win, int i)
{
    float v = KeyElem<T>::one(row + i);
    for (int wi = 1; wi < n_win; ++wi) v = v + KeyElem<T>::one(row + wi * win_stride + i);
    return v;
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kKsThreads) void key_scores_kernel(const KsLaunch L)
{
#pragma clang fp contract(off)
    using P = KeyElem<T>;
    constexpr int E = P::E;
    extern __shared__ __align__(16) unsigned char ks_smem[];
    const int tid = threadIdx.x;
    const int k = blockIdx.x / L.n_chunks, chunk = blockIdx.x - k * L.n_chunks;
    const int OH = L.out_h, OW = L.out_w, on = OH * OW, on4 = ks_tile_floats(OH, OW);
    const int n_tab = ks_tab_entries(OH, OW);
    float* tiles = reinterpret_cast<float*>(ks_smem);            // [batch][on4]
    float* tmp = tiles + (size_t)L.batch * on4;                  // [h][OW] of a staged key
    float* tw = tmp + L.tmp_cap;                                 // [OW + OH][4]: the columns' taps, then the rows'
    int* tix = reinterpret_cast<int*>(tw + n_tab);
    float* wsum = reinterpret_cast<float*>(tix + n_tab);         // [kKsMaskGroup][kKsMaxBatch][4 waves]

    const DaamKeyPlanes key = L.keys[k];
    const int h = key.h, w = key.w, n = h * w, n_win = key.n_win;
    const int64_t ws = key.win_stride;
    const int m_cols = L.n_masks > 0 ? L.n_masks : 1;
    const int t0 = chunk * L.chunk_rows, t1 = t0 + min(L.chunk_rows, L.n_rows - t0);      // t0 < n_rows: n_chunks is the ceiling
    float* out = L.scores + (size_t)k * m_cols * L.n_rows;
    // not a plane: nothing is read.  key_planes_ok() written out: calling it here compiles to other machine code than the profiled one
    if (h < 1 || h > kKeyMaxSide || w < 1 || w > kKeyMaxSide || n_win < 1) {
        const int nt = t1 - t0;
        for (int i = tid; i < m_cols * nt; i += kKsThreads) out[(size_t)(i / nt) * L.n_rows + t0 + i % nt] = NAN;
        return;
    }
    const bool same = h == OH && w == OW;
    const bool staged = !same && n <= on && h * OW <= L.tmp_cap;
    if (!same) {
        for (int i = tid; i < OW + OH; i += kKsThreads) {
            const bool is_x = i < OW;
            const int n_in = is_x ? w : h, n_out = is_x ? OW : OH;
            float wt[4];
            const int first = cubic_taps((float)n_in / (float)n_out, is_x ? i : i - OW, wt);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                tix[i * 4 + a] = min(max(first + a, 0), n_in - 1);
                tw[i * 4 + a] = wt[a];
            }
        }
    }
    const T* base = reinterpret_cast<const T*>(key.base);
    // 16-byte pieces: whole planes of them from an aligned start, in every window (workgroup-uniform; a row stride of whole pieces
    // keeps every row of the batch aligned with the first)
    const bool pieces = n % E == 0 && (reinterpret_cast<uintptr_t>(base + (size_t)t0 * n) & 15) == 0 &&
                        (n_win == 1 || (ws * (int64_t)sizeof(T)) % 16 == 0);

    for (int tb = t0; tb < t1; tb += L.batch) {
        const int nb = min(L.batch, t1 - tb);
        __syncthreads();                                         // the tables are written; the last batch's dots are done with the tiles
        if (same || staged) {
            for (int b = 0; b < nb; ++b) {
                const T* row = base + (size_t)(tb + b) * n;
                float* dst = tiles + (size_t)b * on4;
                if (pieces) {
                    for (int i = tid; i < n / E; i += kKsThreads) {
                        typename P::Piece p = as_global<typename P::Piece>(row)[i];
                        float v[E];
#pragma unroll
                        for (int e = 0; e < E; ++e) v[e] = P::at(p, e);
                        for (int wi = 1; wi < n_win; ++wi) {
                            p = as_global<typename P::Piece>(row + wi * ws)[i];
#pragma unroll
                            for (int e = 0; e < E; ++e) v[e] = v[e] + P::at(p, e);
                        }
#pragma unroll
                        for (int e = 0; e < E; e += 4) {
                            float4v q = {v[e], v[e + 1], v[e + 2], v[e + 3]};
                            if (same) q = float4v{fmaxf(q[0], 0.f), fmaxf(q[1], 0.f), fmaxf(q[2], 0.f), fmaxf(q[3], 0.f)};
                            *reinterpret_cast<float4v*>(dst + i * E + e) = q;
                        }
                    }
                } else {
                    for (int i = tid; i < n; i += kKsThreads) {
                        const float v = ks_elem<T>(row, ws, n_win, i);
                        dst[i] = same ? fmaxf(v, 0.f) : v;
                    }
                }
            }
            if (staged) {
                for (int b = 0; b < nb; ++b) {
                    float* tile = tiles + (size_t)b * on4;
                    __syncthreads();                             // the planes have landed; the last row's column pass is done with tmp
                    for (int i = tid; i < h * OW; i += kKsThreads) {
                        const int y = i / OW, ox = i - y * OW;
                        tmp[i] = cubic_row(tile + y * w, tix + ox * 4, tw + ox * 4);
                    }
                    __syncthreads();                             // ... and every lane is done with the plane the tile now replaces
                    for (int i = tid; i < on; i += kKsThreads) {
                        const int oy = i / OW, ox = i - oy * OW;
                        const int* iy = tix + (OW + oy) * 4;
                        const float* wy = tw + (OW + oy) * 4;
                        const float v = tmp[iy[0] * OW + ox] * wy[0] + tmp[iy[1] * OW + ox] * wy[1] + tmp[iy[2] * OW + ox] * wy[2] +
                                        tmp[iy[3] * OW + ox] * wy[3];
                        tile[i] = fmaxf(v, 0.f);
                    }
                }
            }
        } else {
            for (int b = 0; b < nb; ++b) {
                const T* row = base + (size_t)(tb + b) * n;
                float* tile = tiles + (size_t)b * on4;
                for (int i = tid; i < on; i += kKsThreads) {
                    const int oy = i / OW, ox = i - oy * OW;
                    const int* ix = tix + ox * 4;
                    const float* wx = tw + ox * 4;
                    const int* iy = tix + (OW + oy) * 4;
                    const float* wy = tw + (OW + oy) * 4;
                    float r[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int at = iy[a] * w;
                        r[a] = ks_elem<T>(row, ws, n_win, at + ix[0]) * wx[0] + ks_elem<T>(row, ws, n_win, at + ix[1]) * wx[1] +
                               ks_elem<T>(row, ws, n_win, at + ix[2]) * wx[2] + ks_elem<T>(row, ws, n_win, at + ix[3]) * wx[3];
                    }
                    tile[i] = fmaxf(r[0] * wy[0] + r[1] * wy[1] + r[2] * wy[2] + r[3] * wy[3], 0.f);
                }
            }
        }
        __syncthreads();

        // dots: row b of the batch against the footprints m0 .. m0 + 3; a row's chain does not know its place in the batch
        for (int m0 = 0; m0 < m_cols; m0 += kKsMaskGroup) {
            const int nm = min(kKsMaskGroup, m_cols - m0);
            float acc[kKsMaskGroup][kKsMaxBatch];
#pragma unroll
            for (int mi = 0; mi < kKsMaskGroup; ++mi)
#pragma unroll
                for (int b = 0; b < kKsMaxBatch; ++b) acc[mi][b] = 0.f;
            for (int p = tid; p < on; p += kKsThreads) {
                float f[kKsMaskGroup], tv[kKsMaxBatch];
#pragma unroll
                for (int mi = 0; mi < kKsMaskGroup; ++mi)
                    f[mi] = mi >= nm ? 0.f : (L.footprint ? as_global<float>(L.footprint)[(size_t)(m0 + mi) * on + p] : 1.0f);
#pragma unroll
                for (int b = 0; b < kKsMaxBatch; ++b) tv[b] = b < nb ? tiles[(size_t)b * on4 + p] : 0.f;
#pragma unroll
                for (int mi = 0; mi < kKsMaskGroup; ++mi)
#pragma unroll
                    for (int b = 0; b < kKsMaxBatch; ++b) acc[mi][b] = __builtin_fmaf(f[mi], tv[b], acc[mi][b]);
            }
#pragma unroll
            for (int mi = 0; mi < kKsMaskGroup; ++mi) {
                if (mi >= nm) continue;
#pragma unroll
                for (int b = 0; b < kKsMaxBatch; ++b) {
                    if (b >= nb) continue;
                    float v = acc[mi][b];
                    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
                    if ((tid & 63) == 0) wsum[(mi * kKsMaxBatch + b) * 4 + (tid >> 6)] = v;
                }
            }
            __syncthreads();
            if (tid < nm * nb) {
                const int mi = tid / nb, b = tid - mi * nb;
                const float* s = wsum + (mi * kKsMaxBatch + b) * 4;
                out[(size_t)(m0 + mi) * L.n_rows + tb + b] = (s[0] + s[1]) + (s[2] + s[3]);
            }
            __syncthreads();                                     // the next group writes wsum again
        }
    }
}

// the library's one error buffer and the entry points' shared checks (daam_key_planes.h)
static thread_local char analysis_error[256] = "";

int analysis_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(analysis_error, sizeof(analysis_error), fmt, ap);
    va_end(ap);
    return code;
}

int key_args_check(int n_keys, int dtype, int n_rows, int max_rows, bool null_arg)
{
    if (n_keys < 1 || n_keys > kKeyMaxKeys) return analysis_fail(DAAM_E_INVALID, "%d keys: 1..%d", n_keys, kKeyMaxKeys);
    if (max_rows && (n_rows < 1 || n_rows > max_rows)) return analysis_fail(DAAM_E_INVALID, "%d token rows: 1..%d", n_rows, max_rows);
    if (n_rows < 1) return analysis_fail(DAAM_E_INVALID, "%d token rows: at least 1", n_rows);
    if (dtype != DAAM_F16 && dtype != DAAM_F32 && dtype != DAAM_BF16) return analysis_fail(DAAM_E_INVALID, "dtype %d: f16, f32 or bf16", dtype);
    if (null_arg) return analysis_fail(DAAM_E_INVALID, "NULL argument");
    return 0;
}

}  // namespace daam

using namespace daam;

int daam_analysis_abi_version(void) { return DAAM_ANALYSIS_ABI_VERSION; }

const char* daam_analysis_last_error(void) { return analysis_error; }

int daam_key_scores(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, int out_h, int out_w, const float* footprint,
                    int n_masks, float* scores, void* stream)
{
    if (key_args_check(n_keys, dtype, n_rows, 0, !keys || !scores)) return DAAM_E_INVALID;
    if (n_masks < 0 || n_masks > kKsMaxMasks) return analysis_fail(DAAM_E_INVALID, "%d masks: 0..%d", n_masks, kKsMaxMasks);
    if (out_h < 1 || out_h > kKeyMaxSide || out_w < 1 || out_w > kKeyMaxSide)
        return analysis_fail(DAAM_E_INVALID, "output of %d x %d: 1 <= out_h, out_w <= %d", out_h, out_w, kKeyMaxSide);
    if ((footprint == nullptr) != (n_masks == 0))
        return analysis_fail(DAAM_E_INVALID, "footprint must be NULL exactly when n_masks is 0 (got %d masks)", n_masks);

    KsLaunch L;
    L.keys = keys; L.footprint = footprint; L.scores = scores;
    L.n_keys = n_keys; L.n_rows = n_rows; L.out_h = out_h; L.out_w = out_w; L.n_masks = n_masks;
    L.tmp_cap = ks_tmp_floats(out_h, out_w);
    // the largest batch that leaves room for a second workgroup on the CU; failing that, the largest that fits at all
    L.batch = 0;
    for (int b = kKsMaxBatch; b >= 1 && !L.batch; --b)
        if (ks_lds_bytes(out_h, out_w, b) <= kKsTwoPerCu) L.batch = b;
    for (int b = kKsMaxBatch; b >= 1 && !L.batch; --b)
        if (ks_lds_bytes(out_h, out_w, b) <= kKsMaxLds) L.batch = b;
    if (!L.batch)
        return analysis_fail(DAAM_E_UNSUPPORTED, "an output of %d x %d needs %zu bytes of LDS, more than %zu", out_h, out_w, ks_lds_bytes(out_h, out_w, 1), kKsMaxLds);
    // two batches per workgroup, more where the grid would not hold n_keys x chunks
    const int64_t max_chunks = 0x7fffffffll / n_keys;
    int64_t chunk_rows = 2 * L.batch;
    const int64_t need = (n_rows + max_chunks - 1) / max_chunks;
    if (need > chunk_rows) chunk_rows = (need + L.batch - 1) / L.batch * L.batch;
    L.chunk_rows = (int32_t)(chunk_rows < n_rows ? chunk_rows : n_rows);                  // (one chunk: as many rows as there are)
    L.n_chunks = (int32_t)((n_rows + (int64_t)L.chunk_rows - 1) / L.chunk_rows);
    const size_t lds = ks_lds_bytes(out_h, out_w, L.batch);
    const dim3 grid((unsigned)((int64_t)n_keys * L.n_chunks));
    const hipError_t e = fin_dispatch(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return fin_launch(key_scores_kernel<T>, grid, kKsThreads, lds, (hipStream_t)stream, L);
    });
    if (e != hipSuccess) return analysis_fail((int)e, "key scores: %s", hipGetErrorString(e));
    return 0;
}
