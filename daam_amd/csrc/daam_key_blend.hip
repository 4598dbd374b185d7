// daam_key_blend (include/daam_analysis.h): heat maps of up to 8 weighted key sets from one read of the running sums -- the finalize's
// arithmetic per key with a weight in front of the sum over keys.  key_blend_kernel, grid (n_rows x bands, chunks), 256 threads;
// workgroup (token row, band of output rows, chunk of 32 keys).  A lane owns one output column and 4 rows of it, lane_rows apart:
// 8 sets x 4 accumulators in registers, its column's taps and its rows' taps in registers too (computed again only when the next
// key has another size); no divide and no table in the loop over keys.  Per key of the chunk that some set weighs:
//   rows        -- the source rows the band's taps reach, read from HBM once, in 16-byte pieces when the plane is a whole number of
//                  them and the address allows (the rule of finalize_rect_kernel; else element by element), windows added in f32
//   row pass    -- tmp[y][ox] = 4 taps along the row, the lane in its own column                         (LDS -> LDS)
//   column pass -- K = max(4 taps down the column of tmp, 0); acc[g][j] += w[g][k] * K for the sets with w != 0   (LDS -> registers)
// A key of the output's size skips the row pass (clamp only).  A key whose rows do not fit the staging (a down-sampling key) gathers
// its 16 taps per output element from global memory, in the same operation order, so the path taken does not show in the bits.
// A key no set weighs is not read; a key that is not a plane is not read and makes the sets that weigh it NaN.  The workgroup writes
// out itself when the call has one chunk; otherwise its tile goes to scratch, for the sets that weigh a key of the chunk, and
// key_blend_join_kernel adds those tiles in chunk order.  No floating-point atomic; contraction off.
#include "daam_key_blend.h"
#include "daam_epilogue.h"

#include <cmath>

namespace daam {

namespace {

// element i of a token row's plane: the windows added in window order
template <typename T> __device__ __forceinline__ float blend_elem(const T* row, int64_t win_stride, int n_win, int i)
{
    float v = KeyElem<T>::one(row + i);
    for (int wi = 1; wi < n_win; ++wi) v = v + KeyElem<T>::one(row + wi * win_stride + i);
    return v;
}

// the clamp at 0 that keeps a NaN (fmaxf would turn it into 0): a set that weighs a key of NaN planes is NaN, as torch's clamp has it
__device__ __forceinline__ float blend_clamp(float v) { return v < 0.f ? 0.f : v; }

// first tap (not clamped) of output index o on an axis of n_in -> n_out
__device__ __forceinline__ int blend_first(int n_in, int n_out, int o)
{
    float unused[4];
    return cubic_taps((float)n_in / (float)n_out, o, unused);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kBlendThreads) void key_blend_kernel(const BlendLaunch L)
{
#pragma clang fp contract(off)
    using P = KeyElem<T>;
    constexpr int E = P::E;
    extern __shared__ __align__(16) unsigned char blend_smem[];
    float* const pl = reinterpret_cast<float*>(blend_smem);      // the plane's rows [ylo, yhi], from element e0 on
    float* const tmp = pl + L.stage_cap;                         // [yhi - ylo + 1][OW]
    float* const wts = tmp + L.stage_cap;                        // [kBlendMaxSets][kBlendChunk]
    const int tid = threadIdx.x;
    const int OH = L.out_h, OW = L.out_w, on = OH * OW;
    const int t = blockIdx.x / L.n_bands, band = blockIdx.x - t * L.n_bands;
    const int chunk = blockIdx.y, k0 = chunk * kBlendChunk, nk = min(kBlendChunk, L.n_keys - k0);
    const int oy0 = band * L.band_h, oy1 = min(oy0 + L.band_h, OH);
    const int tr = tid / OW, ox = tid - tr * OW;                 // the lane's column and its place in the band
    const bool lane_on = tr < L.lane_rows;

    // the chunk's weights; which sets and which keys are in play (workgroup-uniform)
    for (int i = tid; i < kBlendMaxSets * kBlendChunk; i += kBlendThreads) {
        const int g = i / kBlendChunk, kk = i - g * kBlendChunk;
        wts[i] = g < L.n_sets && kk < nk ? as_global<float>(L.weights)[(size_t)g * L.n_keys + k0 + kk] : 0.f;
    }
    __syncthreads();
    unsigned set_mask = 0, key_mask = 0;
    for (int g = 0; g < L.n_sets; ++g)
        for (int kk = 0; kk < nk; ++kk)
            if (wts[g * kBlendChunk + kk] != 0.f) {
                set_mask |= 1u << g;
                key_mask |= 1u << kk;
            }
    if (L.n_chunks > 1) {
        if (blockIdx.x == 0 && tid < L.n_sets) L.flags[tid * L.n_chunks + chunk] = (set_mask >> tid) & 1;
        if (!set_mask) return;                                   // nobody weighs a key of this chunk: nothing is read or written
    }

    float acc[kBlendMaxSets][kBlendRows];
#pragma unroll
    for (int g = 0; g < kBlendMaxSets; ++g)
#pragma unroll
        for (int j = 0; j < kBlendRows; ++j) acc[g][j] = 0.f;

    int ph = 0, pw = 0;                                          // the size the taps in registers belong to
    int ix[4], iy[kBlendRows][4];
    float wx[4], wy[kBlendRows][4];
    int ylo = 0, yhi = 0;

    for (int kk = 0; kk < nk; ++kk) {
        if (!((key_mask >> kk) & 1)) continue;
        const DaamKeyPlanes key = L.keys[k0 + kk];
        const int h = key.h, w = key.w, n_win = key.n_win;
        float kv[kBlendRows];
        if (h < 1 || h > kKeyMaxSide || w < 1 || w > kKeyMaxSide || n_win < 1) {         // not a plane: nothing is read
#pragma unroll
            for (int j = 0; j < kBlendRows; ++j) kv[j] = NAN;
        } else {
            const int n = h * w;
            const int64_t ws = key.win_stride;
            const T* const row = reinterpret_cast<const T*>(key.base) + (size_t)t * n;
            const bool same = h == OH && w == OW;
            if (h != ph || w != pw) {
                ph = h; pw = w;
                const int fx = cubic_taps((float)w / (float)OW, ox, wx);
#pragma unroll
                for (int a = 0; a < 4; ++a) ix[a] = min(max(fx + a, 0), w - 1);
#pragma unroll
                for (int j = 0; j < kBlendRows; ++j) {
                    const int oy = min(oy0 + tr + j * L.lane_rows, oy1 - 1);       // a row past the band repeats its last one
                    const int fy = cubic_taps((float)h / (float)OH, oy, wy[j]);
#pragma unroll
                    for (int a = 0; a < 4; ++a) iy[j][a] = min(max(fy + a, 0), h - 1);
                }
                ylo = same ? oy0 : min(max(blend_first(h, OH, oy0), 0), h - 1);
                yhi = same ? oy1 - 1 : min(max(blend_first(h, OH, oy1 - 1) + 3, 0), h - 1);
            }
            // 16-byte pieces: whole planes of them from an aligned start, in every window (workgroup-uniform)
            const bool pieces = n % E == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0 &&
                                (n_win == 1 || (ws * (int64_t)sizeof(T)) % 16 == 0);
            const int e_lo = ylo * w, e_hi = (yhi + 1) * w;
            const int e0 = pieces ? e_lo / E * E : e_lo;
            const int e1 = pieces ? (e_hi + E - 1) / E * E : e_hi;                       // <= n: the plane is whole pieces
            const int ny = yhi - ylo + 1;
            const bool staged = e1 - e0 <= L.stage_cap && ny * OW <= L.stage_cap;
            if (staged) {
                __syncthreads();                                 // the last key's passes are done with pl and tmp
                if (pieces) {
                    for (int i = tid; i < (e1 - e0) / E; i += kBlendThreads) {
                        typename P::Piece p = as_global<typename P::Piece>(row + e0)[i];
                        float v[E];
#pragma unroll
                        for (int e = 0; e < E; ++e) v[e] = P::at(p, e);
                        for (int wi = 1; wi < n_win; ++wi) {
                            p = as_global<typename P::Piece>(row + wi * ws + e0)[i];
#pragma unroll
                            for (int e = 0; e < E; ++e) v[e] = v[e] + P::at(p, e);
                        }
#pragma unroll
                        for (int e = 0; e < E; e += 4) *reinterpret_cast<float4v*>(pl + i * E + e) = float4v{v[e], v[e + 1], v[e + 2], v[e + 3]};
                    }
                } else {
                    for (int i = tid; i < e1 - e0; i += kBlendThreads) pl[i] = blend_elem<T>(row, ws, n_win, e0 + i);
                }
                __syncthreads();
                if (same) {
                    if (lane_on) {
#pragma unroll
                        for (int j = 0; j < kBlendRows; ++j) {
                            const int oy = min(oy0 + tr + j * L.lane_rows, oy1 - 1);
                            kv[j] = blend_clamp(pl[oy * OW + ox - e0]);
                        }
                    }
                } else {
                    if (lane_on)
                        for (int y = tr; y < ny; y += L.lane_rows) tmp[y * OW + ox] = cubic_row(pl + (ylo + y) * w - e0, ix, wx);
                    __syncthreads();
                    if (lane_on) {
#pragma unroll
                        for (int j = 0; j < kBlendRows; ++j) {
                            const float* col = tmp + ox;
                            const float v = col[(iy[j][0] - ylo) * OW] * wy[j][0] + col[(iy[j][1] - ylo) * OW] * wy[j][1] +
                                            col[(iy[j][2] - ylo) * OW] * wy[j][2] + col[(iy[j][3] - ylo) * OW] * wy[j][3];
                            kv[j] = blend_clamp(v);
                        }
                    }
                }
            } else if (lane_on) {                                // the rows do not fit: 16 taps per element from global memory
#pragma unroll
                for (int j = 0; j < kBlendRows; ++j) {
                    kv[j] = 0.f;
                    if (oy0 + tr + j * L.lane_rows >= oy1) continue;
                    if (same) {
                        kv[j] = blend_clamp(blend_elem<T>(row, ws, n_win, iy[j][1] * w + ix[1]));
                        continue;
                    }
                    float r[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int at = iy[j][a] * w;
                        r[a] = blend_elem<T>(row, ws, n_win, at + ix[0]) * wx[0] + blend_elem<T>(row, ws, n_win, at + ix[1]) * wx[1] +
                               blend_elem<T>(row, ws, n_win, at + ix[2]) * wx[2] + blend_elem<T>(row, ws, n_win, at + ix[3]) * wx[3];
                    }
                    kv[j] = blend_clamp(r[0] * wy[j][0] + r[1] * wy[j][1] + r[2] * wy[j][2] + r[3] * wy[j][3]);
                }
            }
        }
        if (lane_on) {
#pragma unroll
            for (int g = 0; g < kBlendMaxSets; ++g) {
                const float wg = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wts[g * kBlendChunk + kk])));     // wave-uniform
                if (wg != 0.f) {
#pragma unroll
                    for (int j = 0; j < kBlendRows; ++j) acc[g][j] = acc[g][j] + wg * kv[j];
                }
            }
        }
    }

    if (!lane_on) return;
    const bool direct = L.n_chunks == 1;
#pragma unroll
    for (int g = 0; g < kBlendMaxSets; ++g) {
        if (g >= L.n_sets || (!direct && !((set_mask >> g) & 1))) continue;
        float* const dst = (direct ? L.out + (size_t)g * L.set_stride
                                   : L.part + ((size_t)chunk * L.n_sets + g) * L.n_rows * on) + (size_t)t * on;
#pragma unroll
        for (int j = 0; j < kBlendRows; ++j) {
            const int oy = oy0 + tr + j * L.lane_rows;
            if (oy < oy1) dst[oy * OW + ox] = acc[g][j];
        }
    }
}

// out[g] = the tiles of the chunks in which set g weighs a key, added in chunk order; grid (ceil(n_rows * cells / 256), n_sets)
__global__ __launch_bounds__(kBlendThreads) void key_blend_join_kernel(const BlendLaunch L)
{
#pragma clang fp contract(off)
    const int g = blockIdx.y;
    const size_t total = (size_t)L.n_rows * L.out_h * L.out_w;
    const size_t i = (size_t)blockIdx.x * kBlendThreads + threadIdx.x;
    if (i >= total) return;
    float v = 0.f;
    for (int c = 0; c < L.n_chunks; ++c)
        if (L.flags[g * L.n_chunks + c]) v = v + L.part[((size_t)c * L.n_sets + g) * total + i];
    L.out[(size_t)g * L.set_stride + i] = v;
}

namespace {

// the limits both entry points know: 0 when one is out of range
bool blend_sizes_ok(int n_keys, int n_sets, int n_rows, int out_h, int out_w)
{
    if (n_keys < 1 || n_keys > kKeyMaxKeys || n_sets < 1 || n_sets > kBlendMaxSets || n_rows < 1) return false;
    if (out_h < 1 || out_h > kKeyMaxSide || out_w < 1 || out_w > kKeyMaxSide) return false;
    const int band_h = blend_band_h(out_h, out_w), n_bands = (out_h + band_h - 1) / band_h;
    return (int64_t)n_rows * n_bands <= 0x7fffffffll;
}

}  // namespace

}  // namespace daam

using namespace daam;

size_t daam_key_blend_scratch_bytes(int n_keys, int n_sets, int n_rows, int out_h, int out_w)
{
    if (!blend_sizes_ok(n_keys, n_sets, n_rows, out_h, out_w)) return 0;
    return blend_flag_bytes(n_keys, n_sets) + (size_t)blend_chunks(n_keys) * n_sets * n_rows * out_h * out_w * sizeof(float);
}

int daam_key_blend(const DaamKeyPlanes* keys, int n_keys, int dtype, int n_rows, int out_h, int out_w, const float* weights, int n_sets,
                   float* out, int64_t set_stride, void* scratch, size_t scratch_bytes, void* stream)
{
    if (key_args_check(n_keys, dtype, n_rows, 0, !keys || !weights || !out || !scratch)) return DAAM_E_INVALID;
    if (n_sets < 1 || n_sets > kBlendMaxSets) return analysis_fail(DAAM_E_INVALID, "%d weight sets: 1..%d", n_sets, kBlendMaxSets);
    if (out_h < 1 || out_h > kKeyMaxSide || out_w < 1 || out_w > kKeyMaxSide)
        return analysis_fail(DAAM_E_INVALID, "output of %d x %d: 1 <= out_h, out_w <= %d", out_h, out_w, kKeyMaxSide);
    if (!blend_sizes_ok(n_keys, n_sets, n_rows, out_h, out_w))
        return analysis_fail(DAAM_E_INVALID, "%d token rows of %d x %d: more workgroups than a launch grid holds", n_rows, out_h, out_w);
    const int64_t map = (int64_t)n_rows * out_h * out_w;
    if (set_stride < map)
        return analysis_fail(DAAM_E_INVALID, "set_stride %lld: a set is %lld elements", (long long)set_stride, (long long)map);
    const size_t need = daam_key_blend_scratch_bytes(n_keys, n_sets, n_rows, out_h, out_w);
    if (scratch_bytes < need)
        return analysis_fail(DAAM_E_INVALID, "scratch of %zu bytes: %d keys, %d sets, %d rows of %d x %d need %zu", scratch_bytes, n_keys, n_sets,
                             n_rows, out_h, out_w, need);
    const size_t lds = blend_lds_bytes(out_h, out_w);
    if (lds > kBlendMaxLds)
        return analysis_fail(DAAM_E_UNSUPPORTED, "an output of %d x %d needs %zu bytes of LDS, more than %zu", out_h, out_w, lds, kBlendMaxLds);

    BlendLaunch L;
    L.keys = keys; L.weights = weights; L.out = out; L.set_stride = set_stride;
    L.flags = static_cast<int32_t*>(scratch);
    L.part = reinterpret_cast<float*>(static_cast<unsigned char*>(scratch) + blend_flag_bytes(n_keys, n_sets));
    L.n_keys = n_keys; L.n_sets = n_sets; L.n_rows = n_rows; L.out_h = out_h; L.out_w = out_w;
    L.n_chunks = blend_chunks(n_keys);
    L.lane_rows = kBlendThreads / out_w;
    L.band_h = blend_band_h(out_h, out_w);
    L.n_bands = (out_h + L.band_h - 1) / L.band_h;
    L.stage_cap = blend_stage_floats(out_h, out_w);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((int64_t)n_rows * L.n_bands), (unsigned)L.n_chunks);
    hipError_t e = fin_dispatch(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return fin_launch(key_blend_kernel<T>, grid, kBlendThreads, lds, s, L);
    });
    if (e == hipSuccess && L.n_chunks > 1) {
        const dim3 jgrid((unsigned)((map + kBlendThreads - 1) / kBlendThreads), (unsigned)n_sets);
        e = fin_launch(key_blend_join_kernel, jgrid, kBlendThreads, 0, s, L);
    }
    if (e != hipSuccess) return analysis_fail((int)e, "key blend: %s", hipGetErrorString(e));
    return 0;
}
