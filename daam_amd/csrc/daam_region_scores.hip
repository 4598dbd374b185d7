// daam_region_scores: how much of every token row's expanded heat map falls inside each of up to 32 u8 masks, without
// an f32 plane at image resolution.  The bicubic expansion of word_expand[_rect]_kernel under absolute = 1, threshold = 0 is linear,
// so sum_{p set in mask m} E_t[p] = sum_ij F[m][i][j] maps[t][i][j] with F[m] = the mask pulled back through the transpose of the
// resize (its "footprint" on the map's own h x w grid):
//   * region_tables_kernel    : per output row y and column x the first cell its four taps reach and their four weights, clamped taps
//                               folded onto the edge cell (cubic_taps of daam_epilogue.h); zeroes `area`.  Once per call, for all masks.
//   * region_footprint_kernel : a workgroup takes one mask and a band of <= 32 output rows: the band's bytes -> a bit set in LDS (aligned
//                               16-byte loads, bytes at the ends of the stack behind bounds: mask_bits16[_edge] of daam_epilogue.h) and the integer area; x pass: thread (row,
//                               cell j) adds the weights of the row's set pixels that reach j, in ascending x; y pass: thread (cell i, j)
//                               adds weight x row sum over the band's rows in ascending y -> the band's partial, in a window of cell rows
//   * region_combine_kernel   : footprint[m][i][j] = the partials of the bands that reach i, in ascending band order
//   * region_dot_kernel       : scores[g][m][t] = sum_ij footprint[m] maps[g][t], four footprints per workgroup: lane chains, a
//                               butterfly per wave, four waves in order
// No floating-point atomic anywhere: every sum has one order, which depends on the mask's own pixels, H, W, h, w alone -- not on where
// the plane starts in memory, nor on the other masks of the call.  Every product and sum is rounded on its own (contraction off): the
// float64 oracle of tests/_region_domain.py counts the roundings on a term's path.
#include "daam_ctx.h"
#include "daam_epilogue.h"

#include <cmath>

namespace daam {

constexpr int kRsMaxMasks = 32;
constexpr int kRsMaxSide = 128;                // h, w of the maps
constexpr int kRsMaxSets = 65535;              // map sets of one call: the dot kernel's grid.y
constexpr int kRsThreads = 256;
constexpr int kRsDotMasks = 4;                 // footprints per workgroup of the dot pass
constexpr int kRsBandRows = 32;                // rows of a band: the length of a y-pass chain
constexpr int kRsTilePixels = 32768;           // pixels whose bits a workgroup holds at once: a band of whole rows, or a piece of one row
constexpr int kRsBitWords = kRsTilePixels / 32 + 2;      // + the aligned chunks around an unaligned tile

struct RsGeom {
    int H, W, h, w;
    int band;                  // rows per band: min(32, max(1, kRsTilePixels / W))
    int n_bands;
    int win;                   // cell rows a band's partial holds, from the first row's first cell on
    int margin_y, margin_x;    // slack of cell_range
};

struct RsTables {              // device scratch, laid out by rs_tables()
    float* gy;                 // [H][4] folded weights of row y onto the cells by[y] .. by[y] + 3
    float* gx;                 // [W][4]
    int* by;                   // [H]
    int* bx;                   // [W]
    float* part;               // [n_masks][n_bands][win][w]
};

// The output indices [lo, hi) that can reach source cell j of n from an axis of N outputs: a superset of {x : b[x] <= j <= b[x] + 3}
// in integers (src = (n / N)(x + 0.5) - 0.5 in [j - 2, j + 2); the edge cells also take what is clamped onto them).  The passes test
// every index of the range against the table, so the slack costs a compare and no correctness.
__host__ __device__ __forceinline__ void rs_cell_range(int j, int N, int n, int margin, int& lo, int& hi)
{
    const long long a = (long long)(2 * j - 3) * N, b = (long long)(2 * j + 5) * N, d = 2ll * n;
    const long long fl = a >= 0 ? a / d : -((-a + d - 1) / d);
    const long long ce = (b + d - 1) / d;
    const long long l = fl - 1 - margin, r = ce + margin;
    lo = j == 0 ? 0 : (int)(l < 0 ? 0 : (l > N ? N : l));
    hi = j == n - 1 ? N : (int)(r > N ? N : r);
}

// one thread per output row (the first H threads) or column
__global__ __launch_bounds__(kRsThreads) void region_tables_kernel(RsGeom g, RsTables t, uint32_t* area, int n_masks)
{
#pragma clang fp contract(off)
    const long long id = (long long)blockIdx.x * kRsThreads + threadIdx.x;
    if (id < n_masks) area[id] = 0;
    if (id >= (long long)g.H + g.W) return;
    const bool is_y = id < g.H;
    const int o = (int)(is_y ? id : id - g.H);
    const int n_out = is_y ? g.H : g.W, n_in = is_y ? g.h : g.w;
    float* gw = (is_y ? t.gy : t.gx) + 4 * (size_t)o;
    int* gb = (is_y ? t.by : t.bx) + o;
    if (g.H == g.h && g.W == g.w) {            // the expand body's copy path
        *gb = o;
        gw[0] = 1.0f; gw[1] = 0.0f; gw[2] = 0.0f; gw[3] = 0.0f;
        return;
    }
    float wt[4];
    const int first = cubic_taps((float)n_in / (float)n_out, o, wt);
    const int base = min(max(first, 0), n_in - 1);
    float fold[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int k = min(max(first + a, 0), n_in - 1) - base;               // 0 .. 3: the clamp is monotone
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q == k) fold[q] = fold[q] + wt[a];
    }
    *gb = base;
#pragma unroll
    for (int q = 0; q < 4; ++q) gw[q] = fold[q];
}

// grid (n_bands, n_masks)
__global__ __launch_bounds__(kRsThreads) void region_footprint_kernel(const uint8_t* masks, int n_masks, RsGeom g, RsTables t, uint32_t* area)
{
#pragma clang fp contract(off)
    __shared__ uint32_t bits[kRsBitWords];
    __shared__ float rowsum[kRsBandRows * kRsMaxSide];          // [row of the band][cell j]
    __shared__ float gy_s[kRsBandRows * 4];
    __shared__ int by_s[kRsBandRows];
    __shared__ uint32_t count_s;
    const int tid = threadIdx.x;
    const int m = blockIdx.y, band = blockIdx.x;
    const int y0 = band * g.band;
    const int n_rows = min(g.band, g.H - y0);
    const uint8_t* stack_lo = masks;
    const uint8_t* stack_hi = masks + (size_t)n_masks * g.H * g.W;
    const uint8_t* band0 = masks + ((size_t)m * g.H + y0) * g.W;

    for (int i = tid; i < n_rows * g.w; i += kRsThreads) rowsum[i] = 0.0f;
    if (tid < n_rows) {
        by_s[tid] = t.by[y0 + tid];
#pragma unroll
        for (int k = 0; k < 4; ++k) gy_s[4 * tid + k] = t.gy[4 * (size_t)(y0 + tid) + k];
    }
    if (tid == 0) count_s = 0;
    uint32_t count = 0;

    // a band of several rows is one tile; a band of one row wider than a tile is walked piece by piece
    const int row_pixels = g.band > 1 ? g.W * n_rows : g.W;
    for (int x0 = 0; x0 < row_pixels; x0 += kRsTilePixels) {
        const int n_px = min(kRsTilePixels, row_pixels - x0);
        const uint8_t* first = band0 + x0;
        const int shift = (int)(reinterpret_cast<uintptr_t>(first) & 15);
        const uint8_t* chunk0 = first - shift;
        const int n_chunks = (shift + n_px + 15) >> 4;          // <= kRsTilePixels / 16 + 1
        __syncthreads();                                        // the last piece's bits are read, the staging above is written
        uint16_t* halves = reinterpret_cast<uint16_t*>(bits);
        for (int c = tid; c < n_chunks; c += kRsThreads) {
            const uint8_t* p = chunk0 + 16 * (size_t)c;
            const uint32_t b = (p >= stack_lo && p + 16 <= stack_hi) ? mask_bits16(*reinterpret_cast<const uint4*>(p))
                                                                     : mask_bits16_edge(p, stack_lo, stack_hi);
            // the tile's own bytes are [shift, shift + n_px) of the chunks
            const int from = max(shift - 16 * c, 0), to = min(shift + n_px - 16 * c, 16);
            count += __popc(b & ((1u << to) - 1u) & ~((1u << from) - 1u));
            halves[c] = (uint16_t)b;
        }
        if (tid == 0 && (n_chunks & 1)) halves[n_chunks] = 0;   // the word the last chunk half fills
        __syncthreads();

        // x pass: pixel (r, x) is bit shift + r W + x - x0 (r = 0 when the row is walked in pieces)
        const int px_lo = g.band > 1 ? 0 : x0, px_hi = g.band > 1 ? g.W : x0 + n_px;
        for (int item = tid; item < n_rows * g.w; item += kRsThreads) {
            const int r = item / g.w, j = item - r * g.w;
            int xa, xb;
            rs_cell_range(j, g.W, g.w, g.margin_x, xa, xb);
            xa = max(xa, px_lo);
            xb = min(xb, px_hi);
            float acc = rowsum[item];
            int q = shift + r * g.W + (xa - px_lo);
            for (int x = xa; x < xb;) {
                const int n = min(32 - (q & 31), xb - x);
                uint32_t word = bits[q >> 5] >> (q & 31);
                if (n < 32) word &= (1u << n) - 1u;
                while (word) {
                    const int xx = x + __builtin_ctz(word);
                    word &= word - 1u;
                    const int k = j - t.bx[xx];
                    if ((unsigned)k < 4u) acc = acc + t.gx[4 * (size_t)xx + k];
                }
                x += n;
                q += n;
            }
            rowsum[item] = acc;
        }
    }
    __syncthreads();

    // y pass: the band's partial on the cell rows [by of its first row, + win)
    const int i0 = by_s[0];
    float* part = t.part + ((size_t)m * g.n_bands + band) * g.win * g.w;
    for (int item = tid; item < g.win * g.w; item += kRsThreads) {
        const int il = item / g.w, j = item - il * g.w;
        const int i = i0 + il;
        float acc = 0.0f;
        for (int r = 0; r < n_rows; ++r) {
            const int k = i - by_s[r];
            if ((unsigned)k < 4u) acc = acc + gy_s[4 * r + k] * rowsum[r * g.w + j];
        }
        part[item] = acc;
    }

    // the area: integers, any order
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if ((tid & 63) == 0 && count) atomicAdd(&count_s, count);
    __syncthreads();
    if (tid == 0 && count_s) atomicAdd(&area[m], count_s);
}

// one thread per cell of every footprint
__global__ __launch_bounds__(kRsThreads) void region_combine_kernel(int n_masks, RsGeom g, RsTables t, float* footprint)
{
#pragma clang fp contract(off)
    const int cells = g.h * g.w;
    const int id = blockIdx.x * kRsThreads + threadIdx.x;
    if (id >= n_masks * cells) return;
    const int m = id / cells, c = id - m * cells;
    const int i = c / g.w, j = c - i * g.w;
    int ya, yb;
    rs_cell_range(i, g.H, g.h, g.margin_y, ya, yb);
    float acc = 0.0f;
    if (ya < yb) {
        const int b1 = (yb - 1) / g.band;
        for (int b = ya / g.band; b <= b1; ++b) {
            const int il = i - t.by[b * g.band];
            if ((unsigned)il < (unsigned)g.win) acc = acc + t.part[(((size_t)m * g.n_bands + b) * g.win + il) * g.w + j];
        }
    }
    footprint[id] = acc;
}

// grid (rows, n_sets, groups of kRsDotMasks footprints): a workgroup holds one map row against the footprints of its group
__global__ __launch_bounds__(kRsThreads) void region_dot_kernel(const float* footprint, int n_masks, const float* maps, int rows, int cells,
                                                                 float* scores)
{
#pragma clang fp contract(off)
    __shared__ float wave_sums[kRsDotMasks][kRsThreads / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x, set = blockIdx.y, m0 = blockIdx.z * kRsDotMasks;
    const int n_here = min(kRsDotMasks, n_masks - m0);
    const float* v = maps + ((size_t)set * rows + row) * cells;
    for (int m = 0; m < n_here; ++m) {
        const float* f = footprint + (size_t)(m0 + m) * cells;
        float acc = 0.0f;
        for (int c = tid; c < cells; c += kRsThreads) acc = acc + f[c] * v[c];
        for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if ((tid & 63) == 0) wave_sums[m][tid >> 6] = acc;
    }
    __syncthreads();
    if (tid < n_here)
        scores[((size_t)set * n_masks + m0 + tid) * rows + row] = (wave_sums[tid][0] + wave_sums[tid][1]) + (wave_sums[tid][2] + wave_sums[tid][3]);
}

// the limits both entry points share: the footprints' shape, and the map sets of a dot pass (its grid.y, grid.x)
static bool rs_footprints_ok(int n_masks, int h, int w)
{
    return n_masks >= 1 && n_masks <= kRsMaxMasks && h >= 1 && h <= kRsMaxSide && w >= 1 && w <= kRsMaxSide;
}
static bool rs_sets_ok(int n_sets, int rows) { return n_sets >= 1 && n_sets <= kRsMaxSets && rows >= 1; }

static void launch_dots(const float* footprint, int n_masks, const float* maps, int n_sets, int rows, int cells, float* scores, hipStream_t s)
{
    hipLaunchKernelGGL(region_dot_kernel, dim3(rows, n_sets, (n_masks + kRsDotMasks - 1) / kRsDotMasks), dim3(kRsThreads), 0, s, footprint,
                       n_masks, maps, rows, cells, scores);
}

static bool rs_geometry(int n_masks, int H, int W, int h, int w, RsGeom& g)
{
    if (!rs_footprints_ok(n_masks, h, w)) return false;
    if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return false;
    g.H = H; g.W = W; g.h = h; g.w = w;
    g.band = W >= kRsTilePixels ? 1 : (kRsTilePixels / W < kRsBandRows ? kRsTilePixels / W : kRsBandRows);
    g.n_bands = (H + g.band - 1) / g.band;
    // a band's rows reach the cells from by[first] to by[last] + 3, and by[last] - by[first] <= ceil((h / H)(band - 1)) + 1
    const long long reach = ((long long)h * g.band + H - 1) / H + 6;
    g.win = (int)(reach < h ? reach : h);
    g.margin_y = 1 + (H >> 20);
    g.margin_x = 1 + (W >> 20);
    return true;
}

static size_t rs_tables(const RsGeom& g, int n_masks, void* workspace, RsTables* t)
{
    size_t at = 0;
    char* base = static_cast<char*>(workspace);
    auto take = [&](size_t bytes) { char* p = base ? base + at : nullptr; at += (bytes + 15) & ~(size_t)15; return p; };
    float* gy = reinterpret_cast<float*>(take(16 * (size_t)g.H));
    float* gx = reinterpret_cast<float*>(take(16 * (size_t)g.W));
    int* by = reinterpret_cast<int*>(take(4 * (size_t)g.H));
    int* bx = reinterpret_cast<int*>(take(4 * (size_t)g.W));
    float* part = reinterpret_cast<float*>(take(4 * (size_t)n_masks * g.n_bands * g.win * g.w));
    if (t) { t->gy = gy; t->gx = gx; t->by = by; t->bx = bx; t->part = part; }
    return at;
}

}  // namespace daam

size_t daam_region_scores_workspace(int n_masks, int H, int W, int h, int w)
{
    RsGeom g;
    if (!rs_geometry(n_masks, H, W, h, w, g)) return 0;
    return rs_tables(g, n_masks, nullptr, nullptr);
}

int daam_region_scores(const uint8_t* masks, int n_masks, int H, int W, const float* maps, int n_sets, int rows, int h, int w,
                       float* footprint, float* scores, uint32_t* area, void* workspace, void* stream)
{
    RsGeom g;
    if (!rs_geometry(n_masks, H, W, h, w, g))
        return fail(DAAM_E_INVALID, "%d masks of %d x %d onto maps of %d x %d: 1..%d masks, 1 <= h, w <= %d, 1 <= H, W, H * W < 2^31",
                    n_masks, H, W, h, w, kRsMaxMasks, kRsMaxSide);
    if (!masks || !footprint || !area || !workspace) return fail(DAAM_E_INVALID, "NULL argument");
    if ((maps == nullptr) != (scores == nullptr)) return fail(DAAM_E_INVALID, "maps and scores: both or neither");
    if (maps && !rs_sets_ok(n_sets, rows)) return fail(DAAM_E_INVALID, "%d sets of %d rows", n_sets, rows);
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(DAAM_E_INVALID, "workspace is not 16-byte aligned");
    if ((long long)g.n_bands > 0x7fffffffll || ((long long)H + W + kRsThreads - 1) / kRsThreads > 0x7fffffffll)
        return fail(DAAM_E_INVALID, "bad mask size %d x %d", H, W);
    RsTables t;
    rs_tables(g, n_masks, workspace, &t);
    hipStream_t s = (hipStream_t)stream;
    const int n_tab = H + W > n_masks ? H + W : n_masks;      // H + W < 2^31 + 1: H * W < 2^31
    hipLaunchKernelGGL(region_tables_kernel, dim3((n_tab + kRsThreads - 1) / kRsThreads), dim3(kRsThreads), 0, s, g, t, area, n_masks);
    hipLaunchKernelGGL(region_footprint_kernel, dim3(g.n_bands, n_masks), dim3(kRsThreads), 0, s, masks, n_masks, g, t, area);
    hipLaunchKernelGGL(region_combine_kernel, dim3((n_masks * h * w + kRsThreads - 1) / kRsThreads), dim3(kRsThreads), 0, s, n_masks, g, t,
                       footprint);
    if (maps) launch_dots(footprint, n_masks, maps, n_sets, rows, h * w, scores, s);
    return launched("region scores");
}

int daam_region_dots(const float* footprint, int n_masks, const float* maps, int n_sets, int rows, int h, int w, float* scores, void* stream)
{
    if (!footprint || !maps || !scores) return fail(DAAM_E_INVALID, "NULL argument");
    if (!rs_footprints_ok(n_masks, h, w))
        return fail(DAAM_E_INVALID, "%d footprints of %d x %d: 1..%d, 1 <= h, w <= %d", n_masks, h, w, kRsMaxMasks, kRsMaxSide);
    if (!rs_sets_ok(n_sets, rows)) return fail(DAAM_E_INVALID, "%d sets of %d rows", n_sets, rows);
    launch_dots(footprint, n_masks, maps, n_sets, rows, h * w, scores, (hipStream_t)stream);
    return launched("region dots");
}
