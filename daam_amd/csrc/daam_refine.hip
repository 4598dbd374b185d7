// daam_refine_affinity / daam_refine_apply (include/daam_refine.h): local-affinity propagation of soft word maps along the image's
// colour affinities.  A workgroup of 256 threads owns a tile of 4 rows x 64 columns, one wave per row and one pixel
// per lane, so every access of a wave to a plane is 64 consecutive elements: the weights [K][h][w] (k-major: for a fixed k a wave
// reads 256 contiguous bytes), the maps, and the neighbours, which for an offset (dy, dx) * d are the same 64 elements shifted by
// dx * d (and folded onto the border where the clamp bites).  The halo of a tile reaches 64 pixels to every side, far more than
// the tile itself, so neighbours are gathered from global memory and served by the vector L1 and the L2; LDS is not used.
//   * refine_affinity_kernel<C> : per pixel the integer sums of the K + 1 samples and of their squares (exact), the deviation from
//                                 n * S2 - S1^2, then three walks over the neighbours: the largest logit, the sum of exponentials,
//                                 the weights.  The image (h w C bytes) stays in cache; K h w floats are written once.
//   * refine_apply_kernel<NMAX> : one iteration for all maps of a pixel: K weights are fetched once, each feeds n_maps FMAs whose
//                                 accumulators stay in registers (NMAX of them; a call with fewer maps re-reads its last map into
//                                 the spare ones and stores nothing from them).  The last launch also writes masks and labels.
//   * refine_copy_kernel        : iterations == 0: refined = maps, masks and labels from the same values.
// Operation order (the f32 emulation of tests/_refine_domain.py restates it): a_k = -fma(d_2, r_2, fma(d_1, r_1, d_0 * r_0)) with
// d_c = |I_c(q_k) - I_c(p)| an exact integer and r_c = (1 / (255 C)) / fma(scale / (255 n), sqrt(float(n S2_c - S1_c^2)), 1e-8f);
// e_k = expf(a_k - max_k a_k); sum = ((e_0 + e_1) + ...) ascending in k; w_k = e_k / sum.  An iteration is acc = fma(w_k, m(q_k), acc)
// ascending in k from acc = 0.  No atomics, no dependence on the grid: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/daam_refine.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kRfMaxDil = 6;
constexpr int kRfMaxDilation = 64;
constexpr int kRfMaxMaps = 32;
constexpr int kRfMaxIterations = 64;
constexpr int kRfThreads = 256;
constexpr int kRfTileCols = 64;                     // one wave per tile row
constexpr int kRfTileRows = kRfThreads / kRfTileCols;

struct RefineGeom {
    int h, w, n_dil;
    int d[kRfMaxDil];
    unsigned tiles_x;
};

// The pixel of this thread; false past the image.  Tiles are numbered row-major in a 1-D grid (h may exceed what grid.y takes).
__device__ __forceinline__ bool refine_pixel(const RefineGeom& g, int& y, int& x)
{
    const unsigned ty = blockIdx.x / g.tiles_x, tx = blockIdx.x - ty * g.tiles_x;
    x = (int)(tx * kRfTileCols + (threadIdx.x & (kRfTileCols - 1)));
    y = (int)(ty * kRfTileRows + threadIdx.x / kRfTileCols);
    return x < g.w && y < g.h;
}

// The eight neighbours of (y, x) at dilation d as indices into a plane, in the header's order, clamped to the image.
__device__ __forceinline__ void refine_neighbours(const RefineGeom& g, int y, int x, int d, int (&q)[8])
{
    const int ym = max(y - d, 0) * g.w, y0 = y * g.w, yp = min(y + d, g.h - 1) * g.w;
    const int xm = max(x - d, 0), xp = min(x + d, g.w - 1);
    q[0] = ym + xm; q[1] = ym + x; q[2] = ym + xp;
    q[3] = y0 + xm;                q[4] = y0 + xp;
    q[5] = yp + xm; q[6] = yp + x; q[7] = yp + xp;
}

template <int C>
__device__ __forceinline__ float refine_logit(const uint8_t* __restrict__ image, int q, const int (&centre)[C], const float (&r)[C])
{
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int v = image[(size_t)q * C + c];
        const float d = (float)abs(v - centre[c]);
        t = c == 0 ? d * r[0] : __fmaf_rn(d, r[c], t);
    }
    return -t;
}

template <int C>
__global__ __launch_bounds__(kRfThreads) void refine_affinity_kernel(const uint8_t* __restrict__ image, float* __restrict__ weights,
                                                                      RefineGeom g, float dev_scale, float chan_scale)
{
    int y, x;
    if (!refine_pixel(g, y, x)) return;
    const int p = y * g.w + x;
    const size_t plane = (size_t)g.h * g.w;
    int centre[C], s1[C], s2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        centre[c] = image[(size_t)p * C + c];
        s1[c] = centre[c];
        s2[c] = centre[c] * centre[c];
    }
    int q[8];
    for (int di = 0; di < g.n_dil; ++di) {
        refine_neighbours(g, y, x, g.d[di], q);
#pragma unroll
        for (int o = 0; o < 8; ++o)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int v = image[(size_t)q[o] * C + c];
                s1[c] += v;
                s2[c] += v * v;
            }
    }
    const int n = 8 * g.n_dil + 1;                      // <= 49: n * s2 <= 49 * 49 * 255^2 < 2^31
    float r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = chan_scale / __fmaf_rn(dev_scale, __fsqrt_rn((float)(n * s2[c] - s1[c] * s1[c])), 1e-8f);

    float top = -INFINITY;
    for (int di = 0; di < g.n_dil; ++di) {
        refine_neighbours(g, y, x, g.d[di], q);
#pragma unroll
        for (int o = 0; o < 8; ++o) top = fmaxf(top, refine_logit<C>(image, q[o], centre, r));
    }
    float sum = 0.f;
    for (int di = 0; di < g.n_dil; ++di) {
        refine_neighbours(g, y, x, g.d[di], q);
#pragma unroll
        for (int o = 0; o < 8; ++o) sum += expf(refine_logit<C>(image, q[o], centre, r) - top);
    }
    float* out = weights + p;
    for (int di = 0; di < g.n_dil; ++di) {
        refine_neighbours(g, y, x, g.d[di], q);
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            *out = expf(refine_logit<C>(image, q[o], centre, r) - top) / sum;
            out += plane;
        }
    }
}

// What the last launch adds to `refined`: the masks and the label of the pixel from the values just stored.
template <int NMAX>
__device__ __forceinline__ void refine_store(const float (&v)[NMAX], int n_maps, size_t plane, int p, float threshold, float* __restrict__ dst,
                                             uint8_t* __restrict__ masks, uint8_t* __restrict__ labels, bool last)
{
    float best = v[0];
    int owner = 0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
        if (j < n_maps) {
            dst[j * plane + p] = v[j];
            if (last && masks) masks[j * plane + p] = v[j] > threshold ? 1 : 0;
            if (v[j] > best) {
                best = v[j];
                owner = j;
            }
        }
    if (last && labels) labels[p] = best > threshold ? (uint8_t)owner : (uint8_t)255;
}

template <int NMAX>
__global__ __launch_bounds__(kRfThreads) void refine_apply_kernel(const float* __restrict__ weights, const float* __restrict__ src,
                                                                   float* __restrict__ dst, uint8_t* __restrict__ masks,
                                                                   uint8_t* __restrict__ labels, RefineGeom g, int n_maps, float threshold,
                                                                   int last)
{
    int y, x;
    if (!refine_pixel(g, y, x)) return;
    const int p = y * g.w + x;
    const size_t plane = (size_t)g.h * g.w;
    const float* maps[NMAX];                            // wave-uniform; spare slots re-read the last map
#pragma unroll
    for (int j = 0; j < NMAX; ++j) maps[j] = src + (size_t)min(j, n_maps - 1) * plane;
    float acc[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) acc[j] = 0.f;
    const float* wk = weights + p;
    int q[8];
    for (int di = 0; di < g.n_dil; ++di) {
        refine_neighbours(g, y, x, g.d[di], q);
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const float wv = *wk;
            wk += plane;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) acc[j] = __fmaf_rn(wv, maps[j][q[o]], acc[j]);
        }
    }
    refine_store<NMAX>(acc, n_maps, plane, p, threshold, dst, masks, labels, last != 0);
}

__global__ __launch_bounds__(kRfThreads) void refine_copy_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                  uint8_t* __restrict__ masks, uint8_t* __restrict__ labels, RefineGeom g,
                                                                  int n_maps, float threshold)
{
    int y, x;
    if (!refine_pixel(g, y, x)) return;
    const int p = y * g.w + x;
    const size_t plane = (size_t)g.h * g.w;
    float best = src[p];
    int owner = 0;
    for (int j = 0; j < n_maps; ++j) {
        const float v = src[j * plane + p];
        dst[j * plane + p] = v;
        if (masks) masks[j * plane + p] = v > threshold ? 1 : 0;
        if (v > best) {
            best = v;
            owner = j;
        }
    }
    if (labels) labels[p] = best > threshold ? (uint8_t)owner : (uint8_t)255;
}

namespace {

thread_local char refine_error[256] = "";

int refine_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int refine_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(refine_error, sizeof(refine_error), fmt, ap);
    va_end(ap);
    return code;
}

bool refine_size_ok(int h, int w, int n_dil)
{
    return n_dil >= 1 && n_dil <= kRfMaxDil && h >= 1 && w >= 1 && 8ll * n_dil * h * w < (1ll << 31);
}

// The checks both calls share; fills the geometry.  0 = ok.
int refine_geometry(const char* who, int h, int w, const int32_t* dilations, int n_dil, RefineGeom& g)
{
    if (n_dil < 1 || n_dil > kRfMaxDil) return refine_fail(DAAM_E_INVALID, "%s: %d dilations: 1..%d", who, n_dil, kRfMaxDil);
    if (h < 1 || w < 1 || !refine_size_ok(h, w, n_dil))
        return refine_fail(DAAM_E_INVALID, "%s: %d x %d with %d dilations: at least 1 x 1, fewer than 2^31 weights", who, h, w, n_dil);
    if (!dilations) return refine_fail(DAAM_E_INVALID, "%s: NULL dilations", who);
    for (int i = 0; i < n_dil; ++i) {
        if (dilations[i] < 1 || dilations[i] > kRfMaxDilation || (i && dilations[i] <= dilations[i - 1]))
            return refine_fail(DAAM_E_INVALID, "%s: dilation %d at position %d: strictly increasing within 1..%d", who, dilations[i], i,
                               kRfMaxDilation);
        g.d[i] = dilations[i];
    }
    for (int i = n_dil; i < kRfMaxDil; ++i) g.d[i] = 1;
    g.h = h; g.w = w; g.n_dil = n_dil;
    g.tiles_x = (unsigned)((w + kRfTileCols - 1) / kRfTileCols);
    return 0;
}

// h * w < 2^28, so fewer than 2^27 tiles whatever the shape (w = 1: h / 4 of them)
unsigned refine_tiles(const RefineGeom& g) { return g.tiles_x * (unsigned)((g.h + kRfTileRows - 1) / kRfTileRows); }

size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <int NMAX>
void launch_apply(hipStream_t s, unsigned tiles, const float* weights, const float* src, float* dst, uint8_t* masks, uint8_t* labels,
                  const RefineGeom& g, int n_maps, float threshold, int last)
{
    hipLaunchKernelGGL(refine_apply_kernel<NMAX>, dim3(tiles), dim3(kRfThreads), 0, s, weights, src, dst, masks, labels, g, n_maps,
                       threshold, last);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_refine_abi_version(void) { return DAAM_REFINE_ABI_VERSION; }

const char* daam_refine_last_error(void) { return refine_error; }

size_t daam_refine_weights_bytes(int h, int w, int n_dil)
{
    if (!refine_size_ok(h, w, n_dil)) return 0;
    return sizeof(float) * 8 * (size_t)n_dil * ((size_t)h * w);
}

size_t daam_refine_workspace(int n_maps, int h, int w)
{
    if (n_maps < 1 || n_maps > kRfMaxMaps || !refine_size_ok(h, w, 1)) return 0;
    return round8(sizeof(float) * (size_t)n_maps * ((size_t)h * w));
}

int daam_refine_affinity(const uint8_t* image, int h, int w, int channels, const int32_t* dilations, int n_dil, float scale,
                         float* weights, void* stream)
{
    RefineGeom g;
    if (const int rc = refine_geometry("refine_affinity", h, w, dilations, n_dil, g)) return rc;
    if (channels != 1 && channels != 3) return refine_fail(DAAM_E_INVALID, "refine_affinity: %d channels: 1 or 3", channels);
    if (!std::isfinite(scale) || !(scale > 0.f)) return refine_fail(DAAM_E_INVALID, "refine_affinity: scale %g: finite and > 0", (double)scale);
    if (!image || !weights) return refine_fail(DAAM_E_INVALID, "refine_affinity: image and weights must not be NULL");
    if (reinterpret_cast<uintptr_t>(weights) & 3) return refine_fail(DAAM_E_INVALID, "refine_affinity: weights are not 4-byte aligned");

    const int n = 8 * n_dil + 1;
    const float dev_scale = (float)((double)scale / (255.0 * n));       // sigma = sqrt(n S2 - S1^2) / (255 n)
    const float chan_scale = (float)(1.0 / (255.0 * channels));
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(refine_tiles(g)), block(kRfThreads);
    if (channels == 1) hipLaunchKernelGGL(refine_affinity_kernel<1>, grid, block, 0, s, image, weights, g, dev_scale, chan_scale);
    else hipLaunchKernelGGL(refine_affinity_kernel<3>, grid, block, 0, s, image, weights, g, dev_scale, chan_scale);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return refine_fail((int)e, "refine_affinity: %s", hipGetErrorString(e));
    return 0;
}

int daam_refine_apply(const float* weights, const int32_t* dilations, int n_dil, const float* maps, int n_maps, int h, int w, int iterations,
                      float threshold, float* refined, uint8_t* masks, uint8_t* labels, void* workspace, size_t workspace_bytes, void* stream)
{
    RefineGeom g;
    if (const int rc = refine_geometry("refine_apply", h, w, dilations, n_dil, g)) return rc;
    if (n_maps < 1 || n_maps > kRfMaxMaps) return refine_fail(DAAM_E_INVALID, "refine_apply: %d maps: 1..%d", n_maps, kRfMaxMaps);
    if (iterations < 0 || iterations > kRfMaxIterations)
        return refine_fail(DAAM_E_INVALID, "refine_apply: %d iterations: 0..%d", iterations, kRfMaxIterations);
    if (!std::isfinite(threshold)) return refine_fail(DAAM_E_INVALID, "refine_apply: threshold %g is not finite", (double)threshold);
    if (!weights || !maps || !refined || !workspace)
        return refine_fail(DAAM_E_INVALID, "refine_apply: weights, maps, refined and workspace must not be NULL");
    if ((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(refined) |
         reinterpret_cast<uintptr_t>(workspace)) & 3)
        return refine_fail(DAAM_E_INVALID, "refine_apply: weights, maps, refined and workspace must be 4-byte aligned");
    const size_t need = daam_refine_workspace(n_maps, h, w);
    if (workspace_bytes < need)
        return refine_fail(DAAM_E_INVALID, "refine_apply: workspace of %zu bytes: %d maps of %d x %d need %zu", workspace_bytes, n_maps, h, w, need);
    const size_t bytes = sizeof(float) * (size_t)n_maps * ((size_t)h * w);
    if (overlap(refined, bytes, maps, bytes)) return refine_fail(DAAM_E_INVALID, "refine_apply: refined overlaps maps");
    if (overlap(refined, bytes, workspace, workspace_bytes)) return refine_fail(DAAM_E_INVALID, "refine_apply: refined overlaps the workspace");

    const hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = refine_tiles(g);
    if (iterations == 0) {
        hipLaunchKernelGGL(refine_copy_kernel, dim3(tiles), dim3(kRfThreads), 0, s, maps, refined, masks, labels, g, n_maps, threshold);
    } else {
        float* const scratch = static_cast<float*>(workspace);
        const float* src = maps;
        for (int t = 0; t < iterations; ++t) {
            // the last launch writes refined, the one before it the scratch, and so on back to the first
            float* const dst = (iterations - 1 - t) % 2 == 0 ? refined : scratch;
            const int last = t == iterations - 1;
            if (n_maps <= 1) launch_apply<1>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 2) launch_apply<2>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 3) launch_apply<3>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 4) launch_apply<4>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 6) launch_apply<6>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 8) launch_apply<8>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 12) launch_apply<12>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 16) launch_apply<16>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else if (n_maps <= 24) launch_apply<24>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            else launch_apply<32>(s, tiles, weights, src, dst, masks, labels, g, n_maps, threshold, last);
            src = dst;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return refine_fail((int)e, "refine_apply: %s", hipGetErrorString(e));
    return 0;
}
