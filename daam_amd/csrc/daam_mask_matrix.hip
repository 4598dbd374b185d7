// daam_mask_overlap_matrix: the intersection counts of every mask of one u8 stack with every mask of another (or of the same one)
// and the areas of all of them, in one pass that fetches every mask byte once -- what compute_iou / compute_ioa
// (daam/evaluate.py:14-35) need for all A x B pairs of a Segmentation against truth masks, and WordHeatMap.compute_ioa
// (heatmap.py:95-96) for all word pairs of one prompt.  Integer counts only: no float is accumulated anywhere.
//   * mask_matrix_zero_kernel : the three outputs to zero (the call owns them)
//   * mask_matrix_kernel      : a workgroup of eight waves walks tiles of 1024 pixels.  Per tile a wave turns its planes into bit sets
//                               (a lane: one aligned 16-byte load -> 16 bits, mask_bits16 of daam_epilogue.h) in LDS, then every lane holds a 4 x 4 block of cells
//                               and adds popcount(A_i & B_j) over the tile's 32-bit words.  Cells and areas are summed over the
//                               workgroup's waves in LDS; one global atomic add per non-zero cell and workgroup, at its end.
// The planes are flat: only h * w matters.  A plane may start at any byte: the loads are the aligned 16-byte chunks around it and the
// bit sets are shifted into pixel order afterwards; a chunk that is not wholly inside its stack is read byte by byte behind bounds.
#include "daam_ctx.h"
#include "daam_epilogue.h"

namespace daam {

constexpr int kMmMax = 32;                     // masks per stack
constexpr int kMmTile = 1024;                  // pixels per tile = 64 lanes x 16 bytes
constexpr int kMmWaves = 8;
constexpr int kMmThreads = kMmWaves * 64;
constexpr int kMmSlots = 4;                    // planes a wave loads at once: 64 planes = 8 waves x 2 groups of 4
constexpr int kMmRowWords = kMmTile / 32 + 1;       // a plane's 32 words of one tile, padded: rows 4 apart fall into banks 4 apart
constexpr int kMmWgPerCu = 2;

struct MmArgs {
    const uint8_t* a;
    const uint8_t* b;          // NULL: b = a (rows of a serve both sides)
    int n_a, n_b;
    int n;                     // h * w
    int tiles;
    uint32_t* inter;
    uint32_t* area_a;
    uint32_t* area_b;          // may be NULL when b is
};

// plane m of the two stacks (a's first) at pixel p0: the stack's bytes [lo, hi), the aligned chunk that holds the plane's pixel p0,
// how far into that chunk the pixel lies, and the plane's row in LDS
struct MmPlane { const uint8_t* lo; const uint8_t* hi; const uint8_t* chunk0; int shift; int row; };
__device__ __forceinline__ MmPlane mm_plane(const MmArgs& g, int m, int p0)
{
    const bool in_a = m < g.n_a;
    MmPlane pl;
    pl.lo = in_a ? g.a : g.b;
    pl.hi = pl.lo + (size_t)(in_a ? g.n_a : g.n_b) * g.n;
    const uint8_t* px = pl.lo + (size_t)(in_a ? m : m - g.n_a) * g.n + p0;
    pl.shift = (int)(reinterpret_cast<uintptr_t>(px) & 15);
    pl.chunk0 = px - pl.shift;
    pl.row = in_a ? m : kMmMax + m - g.n_a;
    return pl;
}

__global__ __launch_bounds__(256) void mask_matrix_zero_kernel(MmArgs g)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < g.n_a * g.n_b) g.inter[t] = 0;
    if (t < g.n_a) g.area_a[t] = 0;
    if (t < g.n_b && g.area_b) g.area_b[t] = 0;
}

// kShift: some plane does not start on a 16-byte boundary.  Then a lane also needs the bits of the next chunk (its neighbour's; the
// last lane loads a 65th chunk itself) and shifts the pair down by the plane's misalignment.
template <bool kShift>
__global__ __launch_bounds__(kMmThreads) void mask_matrix_kernel(MmArgs g)
{
    __shared__ uint32_t bits[2][2 * kMmMax * kMmRowWords];      // [buffer][row: 0..31 = a, 32..63 = b][word]
    __shared__ uint32_t cells[kMmMax * kMmMax];
    __shared__ uint32_t areas[2 * kMmMax];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < 2 * 2 * kMmMax * kMmRowWords; i += kMmThreads) (&bits[0][0])[i] = 0;   // rows of no plane stay zero
    for (int i = threadIdx.x; i < kMmMax * kMmMax; i += kMmThreads) cells[i] = 0;
    if (threadIdx.x < 2 * kMmMax) areas[threadIdx.x] = 0;
    __syncthreads();

    const int n_planes = g.n_a + (g.b ? g.n_b : 0);
    const int b_row0 = g.b ? kMmMax : 0;
    const int ib = lane >> 3, jb = lane & 7;                    // the lane's cells: rows 4 ib .., columns 4 jb ..
    const bool active = 4 * ib < g.n_a && 4 * jb < g.n_b;
    uint32_t acc[4][4] = {};
    uint32_t area_rows[4] = {}, area_cols[4] = {};              // popcounts of the lane's four a rows and four b rows

    int buf = 0;
    for (int tile = blockIdx.x; tile < g.tiles; tile += gridDim.x, buf ^= 1) {
        const int p0 = tile * kMmTile;                          // < 2^31: tiles = ceil(n / 1024)
        const int left = g.n - p0 - 16 * lane;                  // pixels of the plane from this lane's first one on
        const uint32_t valid = left >= 16 ? 0xffffu : (left > 0 ? (1u << left) - 1u : 0u);
        uint16_t* rows = reinterpret_cast<uint16_t*>(bits[buf]);
#pragma unroll 1
        for (int m0 = wave; m0 < n_planes; m0 += kMmWaves * kMmSlots) {
            uint4 raw[kMmSlots], extra[kShift ? kMmSlots : 1];
            // the loads of a group of planes are all issued before the first one is waited for
#pragma unroll
            for (int s = 0; s < kMmSlots; ++s) {
                const int m = m0 + kMmWaves * s;
                raw[s] = make_uint4(0, 0, 0, 0);
                if (kShift) extra[s] = make_uint4(0, 0, 0, 0);
                if (m < n_planes) {
                    const MmPlane pl = mm_plane(g, m, p0);
                    const uint8_t* p = pl.chunk0 + 16 * lane;
                    if (p >= pl.lo && p + 16 <= pl.hi) raw[s] = *reinterpret_cast<const uint4*>(p);
                    if (kShift && lane == 63 && pl.shift && p + 16 >= pl.lo && p + 32 <= pl.hi)
                        extra[s] = *reinterpret_cast<const uint4*>(p + 16);
                }
            }
#pragma unroll
            for (int s = 0; s < kMmSlots; ++s) {
                const int m = m0 + kMmWaves * s;
                if (m < n_planes) {
                    const MmPlane pl = mm_plane(g, m, p0);
                    const uint8_t* p = pl.chunk0 + 16 * lane;
                    uint32_t c = (p >= pl.lo && p + 16 <= pl.hi) ? mask_bits16(raw[s]) : mask_bits16_edge(p, pl.lo, pl.hi);
                    if (kShift && pl.shift) {
                        uint32_t next = __shfl_down(c, 1, 64);
                        if (lane == 63)
                            next = (p + 16 >= pl.lo && p + 32 <= pl.hi) ? mask_bits16(extra[s]) : mask_bits16_edge(p + 16, pl.lo, pl.hi);
                        c = ((c | (next << 16)) >> pl.shift) & 0xffffu;
                    }
                    rows[pl.row * kMmRowWords * 2 + lane] = (uint16_t)(c & valid);
                }
            }
        }
        __syncthreads();        // the only barrier of a tile: the next tile writes the other buffer
        if (active) {
            const uint32_t* w = bits[buf];
#pragma unroll
            for (int q = 0; q < kMmTile / 32 / kMmWaves; ++q) {
                const int k = wave + kMmWaves * q;
                uint32_t ra[4], rb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    ra[u] = w[(4 * ib + u) * kMmRowWords + k];
                    rb[u] = w[(b_row0 + 4 * jb + u) * kMmRowWords + k];
                    area_rows[u] += __popc(ra[u]);
                    area_cols[u] += __popc(rb[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] += __popc(ra[u] & rb[v]);
            }
        }
    }

    // the workgroup's sums: LDS atomics over its eight waves, then one global atomic add per non-zero cell
    if (active) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (acc[u][v]) atomicAdd(&cells[(4 * ib + u) * kMmMax + 4 * jb + v], acc[u][v]);
            // every row is held by eight lanes of a wave: the first column block speaks for the a rows, the first row block for b's
            if (jb == 0 && area_rows[u]) atomicAdd(&areas[4 * ib + u], area_rows[u]);
            if (ib == 0 && g.b && area_cols[u]) atomicAdd(&areas[kMmMax + 4 * jb + u], area_cols[u]);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < g.n_a * g.n_b; c += kMmThreads) {
        const int i = c / g.n_b, j = c - i * g.n_b;
        const uint32_t v = cells[i * kMmMax + j];
        if (v) atomicAdd(&g.inter[c], v);
    }
    if ((int)threadIdx.x < g.n_a && areas[threadIdx.x]) atomicAdd(&g.area_a[threadIdx.x], areas[threadIdx.x]);
    if ((int)threadIdx.x < g.n_b && g.area_b && areas[b_row0 + threadIdx.x]) atomicAdd(&g.area_b[threadIdx.x], areas[b_row0 + threadIdx.x]);
}

static int mm_compute_units()
{
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int n = 0;
        cus[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }
    return cus[dev];
}

}  // namespace daam

int daam_mask_overlap_matrix(const uint8_t* a, int n_a, const uint8_t* b, int n_b, int h, int w, uint32_t* inter, uint32_t* area_a,
                             uint32_t* area_b, void* stream)
{
    if (!a || !inter || !area_a) return fail(DAAM_E_INVALID, "NULL argument");
    if (b && !area_b) return fail(DAAM_E_INVALID, "area_b is NULL but b is not");
    if (!b) n_b = n_a;
    if (n_a < 1 || n_a > kMmMax || n_b < 1 || n_b > kMmMax) return fail(DAAM_E_INVALID, "%d x %d masks: 1..%d per stack", n_a, n_b, kMmMax);
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31)) return fail(DAAM_E_INVALID, "bad mask size %d x %d", h, w);
    MmArgs g;
    g.a = a; g.b = b; g.n_a = n_a; g.n_b = n_b;
    g.n = h * w;
    g.tiles = (int)(((long long)g.n + kMmTile - 1) / kMmTile);
    g.inter = inter; g.area_a = area_a; g.area_b = area_b;
    // every plane on a 16-byte boundary: the stacks are, and so is the plane size when a stack has more than one
    bool aligned = (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (n_a == 1 || g.n % 16 == 0);
    if (b) aligned = aligned && (reinterpret_cast<uintptr_t>(b) & 15) == 0 && (n_b == 1 || g.n % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    const int grid = g.tiles < kMmWgPerCu * mm_compute_units() ? g.tiles : kMmWgPerCu * mm_compute_units();
    hipLaunchKernelGGL(mask_matrix_zero_kernel, dim3((n_a * n_b + 255) / 256), dim3(256), 0, s, g);
    if (aligned)
        hipLaunchKernelGGL(mask_matrix_kernel<false>, dim3(grid), dim3(kMmThreads), 0, s, g);
    else
        hipLaunchKernelGGL(mask_matrix_kernel<true>, dim3(grid), dim3(kMmThreads), 0, s, g);
    return launched("mask matrix");
}
