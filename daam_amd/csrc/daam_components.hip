// daam_mask_components (include/daam_components.h): connected components of up to 32 byte masks -- per pixel the rank of its
// component, per mask the number of components, their roots, areas and boxes, the largest one and the cleaned mask -- by union-find
// in LDS and in global memory.  A workgroup owns a tile of 32 rows x 256 columns of one mask; a pixel is named by its
// row-major index y * w + x in its mask, and a parent is always <= its child, so a tree's root is its lowest index.
//   * comp_init_kernel    : the sentinel rows of comps and largest, the largest-component keys and the counts at zero
//   * comp_local_kernel   : the set bits of a tile, 16 bytes at a time -> the tile's components in LDS -> one parent per pixel
//                           (the tile's lowest index of the component; -1 on background), the area at zero at every local root
//   * comp_seam_kernel    : the pixels on a tile's top row and left / right column: their unions with neighbours in other tiles
//   * comp_flatten_kernel : every pixel points at its root; the area joins its root; the roots of every row segment are counted
//   * comp_scan_kernel    : one workgroup per mask: the exclusive scan of the segment counts -> counts[m][0]
//   * comp_roots_kernel   : every root learns its rank (kept in its own parent slot as -2 - rank), writes its comps row's root and
//                           area, joins the largest-component key and counts[m][1]
//   * comp_output_kernel  : labels, kept, the boxes of the listed components and of the largest one
// Which unions are made (neighbour_unions).  For a set pixel p with the neighbours l (left), u (up), ul, ur and r (right):
//   l set -> (p, l);   u set and not (l set and ul set) -> (p, u);   8-connectivity and u clear:  ul set and l clear -> (p, ul);
//   ur set and r clear -> (p, ur).
// That is enough: if l and ul are both set, l is joined to p and (by the same rule at l, by induction on x) to ul, which shares a
// row run with u; with u set, ul and ur share its run; with l set, ul is l's `up`; with r set, ur is r's `up` and r's rule makes
// that union because u, r's `ul`, is clear.  The local kernel makes the unions whose two pixels share a tile (it sees pixels outside
// the tile as clear, which only adds unions) and the seam kernel the others.
// Every loop over parents ends by construction: find steps from x to a parent < x and stops at the first that is not (a
// non-negative integer cannot fall for ever), and unite retries with max(a, b) strictly smaller than before.  No loop waits for
// another thread or workgroup to write something: a lost atomicMin hands back the value that won, and the loop goes on from it.
// Every union hangs the larger root under the smaller (atomicMin), so at the end of the seam kernel every tree's root is its
// component's lowest index whatever the order of the unions: ranks, areas, boxes and the largest component (a 64-bit atomicMax on
// area << 32 | 0xFFFFFFFF - root) are integers joined by integer atomics, and no result depends on the grid or the order.
#include "daam_epilogue.h"
#include "../../include/daam_components.h"

#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kCcMaxMasks = 32;
constexpr int kCcMaxComp = 65536;
constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / 64;
constexpr int kCcTileRows = 32;
constexpr int kCcTileCols = 256;                    // one column per thread
constexpr int kCcRowWords = kCcTileCols / 32;       // a tile row's set bits
constexpr int kCcRowChunks = kCcTileCols / 16 + 1;  // 16-byte aligned chunks that can hold bytes of a tile row at any alignment
constexpr unsigned kCcMaxGrid = 1u << 22;           // workgroups of a launch; larger calls are walked
constexpr size_t kCcHeadBytes = 512;                // the largest-component keys [32] u64, padded

struct CompArgs {
    const uint8_t* masks;
    unsigned long long* key;    // [32]: area << 32 | (0xFFFFFFFF - root); 0 while the mask has no component
    int* parent;                // [n][h * w]: -1 background; the parent's index; from the roots kernel on a root holds -2 - rank
    int* area;                  // [n][h * w]: valid at roots
    int* seg;                   // [n][h * tiles_x]: the roots of a row's 256-column segment, then their exclusive scan
    int32_t* labels;
    int32_t* counts;
    int32_t* comps;
    int32_t* largest;
    uint8_t* kept;
    int n_masks, h, w, conn8, min_area, keep, max_comp;
    unsigned tiles_x, tiles_y, n_tiles, n_seg;      // n_tiles over all masks (<= 2^31), n_seg per mask (< 2^31)
};

struct CompTile {
    int m, y0, col0, n_rows, n_cols;
    unsigned tx;
    size_t base;                // of the mask, in pixels
};

__device__ __forceinline__ CompTile comp_tile(const CompArgs& a, unsigned t)
{
    CompTile tl;
    const unsigned per_mask = a.tiles_x * a.tiles_y;
    tl.m = (int)(t / per_mask);
    const unsigned rem = t - (unsigned)tl.m * per_mask;
    const unsigned ty = rem / a.tiles_x;
    tl.tx = rem - ty * a.tiles_x;
    tl.y0 = (int)ty * kCcTileRows;
    tl.col0 = (int)tl.tx * kCcTileCols;
    tl.n_rows = min(kCcTileRows, a.h - tl.y0);
    tl.n_cols = min(kCcTileCols, a.w - tl.col0);
    tl.base = (size_t)tl.m * ((size_t)a.h * a.w);
    return tl;
}

// ---- union-find; Scope is the memory scope of the parents (LDS: workgroup, global: agent) -----------------------------------------
template <int Scope> __device__ __forceinline__ int uf_find(const int* par, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, Scope);
        if ((unsigned)p >= (unsigned)x) return x;       // a root (p == x); anything else that is not a lower index ends the walk too
        x = p;
    }
}

template <int Scope> __device__ __forceinline__ void uf_unite(int* par, int a, int b)
{
    for (;;) {
        a = uf_find<Scope>(par, a);
        b = uf_find<Scope>(par, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, Scope);
        if ((unsigned)old >= (unsigned)a) return;       // a was a root and now hangs under b
        a = old;                                        // a had got the parent `old` < a meanwhile: old's tree and b's are still to join
    }
}

// the unions of the set pixel (y, x); see the head of the file
template <class IsSet, class Unite>
__device__ __forceinline__ void neighbour_unions(int y, int x, int conn8, bool with_left, IsSet is_set, Unite unite)
{
    const bool l = is_set(y, x - 1), u = is_set(y - 1, x);
    if (l && with_left) unite(y, x - 1);
    if (u) {
        if (!(l && is_set(y - 1, x - 1))) unite(y - 1, x);
    } else if (conn8) {
        if (!l && is_set(y - 1, x - 1)) unite(y - 1, x - 1);
        if (!is_set(y, x + 1) && is_set(y - 1, x + 1)) unite(y - 1, x + 1);
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the runs of a wave's 64 columns of one row: `head` starts a run of lanes that share a root.  The lane of this lane's head, and
// for a head the length of its run
struct WaveRuns {
    unsigned long long heads, set;
    __device__ __forceinline__ int head_lane(int lane) const
    {
        const unsigned long long below = heads & ((2ull << lane) - 1ull);
        return below ? 63 - __builtin_clzll(below) : 0;
    }
    __device__ __forceinline__ int length(int lane) const
    {
        const unsigned long long above = lane == 63 ? 0ull : ((heads | ~set) >> (lane + 1));
        return above ? __builtin_ctzll(above) + 1 : 64 - lane;
    }
};

__global__ __launch_bounds__(kCcThreads) void comp_init_kernel(const CompArgs a)
{
    const size_t rows = (size_t)a.n_masks * a.max_comp;
    const size_t t0 = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
    for (size_t i = t0; i < rows; i += (size_t)gridDim.x * kCcThreads) {
        int32_t* const c = a.comps + 6 * i;
        c[0] = -1; c[1] = 0; c[2] = a.w; c[3] = a.h; c[4] = -1; c[5] = -1;
    }
    if (t0 < (size_t)a.n_masks) {
        int32_t* const c = a.largest + 6 * t0;
        c[0] = -1; c[1] = 0; c[2] = a.w; c[3] = a.h; c[4] = -1; c[5] = -1;
        a.counts[2 * t0] = 0;
        a.counts[2 * t0 + 1] = 0;
        a.key[t0] = 0ull;
    }
}

__global__ __launch_bounds__(kCcThreads) void comp_local_kernel(const CompArgs a)
{
    __shared__ int s_par[kCcTileRows * kCcTileCols];            // local index r * 256 + c: ordered as the global indices are
    __shared__ unsigned s_bits[kCcTileRows][kCcRowWords];
    const int tid = threadIdx.x;
    for (unsigned t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const CompTile tl = comp_tile(a, t);
        s_bits[tid >> 3][tid & 7] = 0u;
        __syncthreads();
        // the tile's bytes, once: whole 16-byte chunks inside the tile's part of a row through mask_bits16, the two that reach over
        // its ends byte by byte (only the tile's own bytes are read)
        const uint8_t* const plane = a.masks + tl.base;
        for (int i = tid; i < kCcTileRows * kCcRowChunks; i += kCcThreads) {
            const int r = i / kCcRowChunks, k = i - r * kCcRowChunks;
            if (r >= tl.n_rows) continue;
            const uint8_t* const rp = plane + (size_t)(tl.y0 + r) * a.w + tl.col0;
            const uint8_t* const re = rp + tl.n_cols;
            const uint8_t* const c = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(rp) & ~(uintptr_t)15) + k * 16;
            if (c >= re) continue;
            uint32_t bits = (c >= rp && c + 16 <= re) ? mask_bits16(*reinterpret_cast<const uint4*>(c)) : mask_bits16_edge(c, rp, re);
            if (!bits) continue;
            int off = (int)(c - rp);                            // -15 .. 255; the set bits are bytes of [rp, re)
            if (off < 0) {
                bits >>= -off;
                off = 0;
            }
            const int word = off >> 5, sh = off & 31;
            atomicOr(&s_bits[r][word], bits << sh);
            if (sh > 16 && word + 1 < kCcRowWords) atomicOr(&s_bits[r][word + 1], bits >> (32 - sh));
        }
        __syncthreads();
        // every set pixel starts at the first pixel of its run inside its 32-bit word
        unsigned colbits = 0;                                   // bit r: pixel (r, tid) is set
        for (int r = 0; r < kCcTileRows; ++r) {
            const unsigned wbits = s_bits[r][tid >> 5];
            const int j = tid & 31;
            const unsigned on = (wbits >> j) & 1u;
            const unsigned clear_below = ~wbits & ((1u << j) - 1u);
            const int start = clear_below ? 32 - __builtin_clz(clear_below) : 0;
            s_par[r * kCcTileCols + tid] = r * kCcTileCols + (on ? (tid & ~31) + start : tid);
            colbits |= on << r;
        }
        __syncthreads();
        for (unsigned rest = colbits; rest; rest &= rest - 1u) {
            const int r = __builtin_ctz(rest);
            neighbour_unions(
                r, tid, a.conn8, (tid & 31) == 0,
                [&](int y, int x) { return y >= 0 && x >= 0 && x < kCcTileCols && ((s_bits[y][x >> 5] >> (x & 31)) & 1u) != 0; },
                [&](int y, int x) {
                    uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, r * kCcTileCols + tid, y * kCcTileCols + x);
                });
        }
        __syncthreads();
        const int x = tl.col0 + tid;
        if (x < a.w) {
            for (int r = 0; r < tl.n_rows; ++r) {
                const size_t g = tl.base + (size_t)(tl.y0 + r) * a.w + x;
                int out = -1;
                if ((colbits >> r) & 1u) {
                    const int me = r * kCcTileCols + tid;
                    const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, me);
                    out = (tl.y0 + (root >> 8)) * a.w + tl.col0 + (root & (kCcTileCols - 1));
                    if (root == me) a.area[g] = 0;              // the roots of the end are among the local roots
                }
                a.parent[g] = out;
            }
        }
        // the next tile's first barrier stands between these reads of s_par / s_bits and its writes
    }
}

__device__ __forceinline__ void seam_pixel(const CompArgs& a, int* par, int y, int x)
{
    const int p = y * a.w + x;
    if (__hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    neighbour_unions(
        y, x, a.conn8, true,
        [&](int qy, int qx) {
            return qy >= 0 && qx >= 0 && qx < a.w && __hip_atomic_load(par + qy * a.w + qx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0;
        },
        [&](int qy, int qx) {
            if ((qy >> 5) != (y >> 5) || (qx >> 8) != (x >> 8)) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, p, qy * a.w + qx);
        });
}

__global__ __launch_bounds__(kCcThreads) void comp_seam_kernel(const CompArgs a)
{
    const int tid = threadIdx.x;
    for (unsigned t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const CompTile tl = comp_tile(a, t);
        int* const par = a.parent + tl.base;
        // the top row: its `up`, `ul` and `ur` lie in the tiles above (and its first pixel's `l` in the tile to the left)
        if (tl.y0 > 0 && tid < tl.n_cols) seam_pixel(a, par, tl.y0, tl.col0 + tid);
        // the rest of the left column (`l`, `ul`) and of the right column (`ur`)
        const int r = tid & 31;
        if (r < tl.n_rows && !(r == 0 && tl.y0 > 0)) {
            if (tid < 32 && tl.col0 > 0) seam_pixel(a, par, tl.y0 + r, tl.col0);
            if (tid >= 32 && tid < 64 && tl.col0 + kCcTileCols < a.w) seam_pixel(a, par, tl.y0 + r, tl.col0 + kCcTileCols - 1);
        }
    }
}

__global__ __launch_bounds__(kCcThreads) void comp_flatten_kernel(const CompArgs a)
{
    __shared__ int s_cnt[kCcTileRows];
    const int tid = threadIdx.x, lane = tid & 63;
    for (unsigned t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const CompTile tl = comp_tile(a, t);
        int* const par = a.parent + tl.base;
        int* const area = a.area + tl.base;
        if (tid < kCcTileRows) s_cnt[tid] = 0;
        __syncthreads();
        const int x = tl.col0 + tid;
        int acc_root = -1, acc_len = 0;                         // a column's runs of one root over consecutive rows: one atomic
        for (int r = 0; r < tl.n_rows; ++r) {
            const int p = (tl.y0 + r) * a.w + min(x, a.w - 1);
            const int v = x < a.w ? __hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
            const int left = __shfl_up(v, 1, 64);
            const bool head = v >= 0 && (lane == 0 || left != v);   // equal parents: one tree
            const WaveRuns runs = {__ballot(head), __ballot(v >= 0)};
            int root = head ? uf_find<__HIP_MEMORY_SCOPE_AGENT>(par, v) : 0;
            root = __shfl(root, runs.head_lane(lane), 64);
            if (v >= 0 && root != v) __hip_atomic_store(par + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (head) {
                const int len = runs.length(lane);
                if (root == acc_root) {
                    acc_len += len;
                } else {
                    if (acc_root >= 0) atomicAdd(area + acc_root, acc_len);
                    acc_root = root;
                    acc_len = len;
                }
            }
            const int n_roots = __popcll(__ballot(head && root == p));  // a root starts a run: its left neighbour has a lower index
            if (lane == 0 && n_roots) atomicAdd(&s_cnt[r], n_roots);
        }
        if (acc_root >= 0) atomicAdd(area + acc_root, acc_len);
        __syncthreads();
        if (tid < tl.n_rows) a.seg[(size_t)tl.m * a.n_seg + (size_t)(tl.y0 + tid) * a.tiles_x + tl.tx] = s_cnt[tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCcThreads) void comp_scan_kernel(const CompArgs a)
{
    __shared__ int s_wave[2][kCcWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* const seg = a.seg + (size_t)blockIdx.x * a.n_seg;
    int carry = 0, buf = 0;
    for (unsigned base = 0; base < a.n_seg; base += kCcThreads, buf ^= 1) {
        const unsigned i = base + tid;
        const int v = i < a.n_seg ? seg[i] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int other = __shfl_up(incl, off, 64);
            if (lane >= off) incl += other;
        }
        if (lane == 63) s_wave[buf][wave] = incl;
        __syncthreads();                                        // two buffers, one barrier per round
        int before = 0, total = 0;
        for (int k = 0; k < kCcWaves; ++k) {
            before += k < wave ? s_wave[buf][k] : 0;
            total += s_wave[buf][k];
        }
        if (i < a.n_seg) seg[i] = carry + before + incl - v;
        carry += total;
    }
    if (tid == 0) a.counts[2 * blockIdx.x] = carry;
}

__global__ __launch_bounds__(kCcThreads) void comp_roots_kernel(const CompArgs a)
{
    __shared__ int s_wc[kCcTileRows][kCcWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (unsigned t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const CompTile tl = comp_tile(a, t);
        int* const par = a.parent + tl.base;
        const int x = tl.col0 + tid;
        unsigned flags = 0;                                     // bit r: pixel (r, tid) is a root
        for (int r = 0; r < tl.n_rows; ++r) {
            const int p = (tl.y0 + r) * a.w + min(x, a.w - 1);
            const bool is_root = x < a.w && par[p] == p;
            const unsigned long long b = __ballot(is_root);
            if (lane == 0) s_wc[r][wave] = __popcll(b);
            flags |= (is_root ? 1u : 0u) << r;
        }
        __syncthreads();
        unsigned long long key = 0ull;
        int big = 0;
        for (int r = 0; r < tl.n_rows; ++r) {
            const bool is_root = (flags >> r) & 1u;
            const unsigned long long b = __ballot(is_root);
            if (is_root) {
                const int p = (tl.y0 + r) * a.w + x;
                int rank = a.seg[(size_t)tl.m * a.n_seg + (size_t)(tl.y0 + r) * a.tiles_x + tl.tx] + __popcll(b & ((1ull << lane) - 1ull));
                for (int k = 0; k < wave; ++k) rank += s_wc[r][k];
                const int ar = a.area[tl.base + p];
                par[p] = -2 - rank;
                if ((unsigned)rank < (unsigned)a.max_comp) {
                    int32_t* const c = a.comps + ((size_t)tl.m * a.max_comp + rank) * 6;
                    c[0] = p;
                    c[1] = ar;
                }
                const unsigned long long mine = ((unsigned long long)(unsigned)ar << 32) | (0xFFFFFFFFu - (unsigned)p);
                key = mine > key ? mine : key;
                big += ar >= a.min_area ? 1 : 0;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(key, off, 64);
            key = other > key ? other : key;
        }
        big = wave_sum(big);
        if (lane == 0 && key) {
            atomicMax(a.key + tl.m, key);
            if (big) atomicAdd(a.counts + 2 * tl.m + 1, big);
        }
        __syncthreads();                                        // s_wc, before the next tile
    }
}

struct CompBox {
    int root, rank, x0, y0, x1, y1;
};

__device__ __forceinline__ void comp_flush_box(const CompArgs& a, int m, int big_root, const CompBox& b)
{
    if (b.root < 0) return;
    if ((unsigned)b.rank < (unsigned)a.max_comp) {
        int32_t* const c = a.comps + ((size_t)m * a.max_comp + b.rank) * 6;
        atomicMin(c + 2, b.x0); atomicMin(c + 3, b.y0); atomicMax(c + 4, b.x1); atomicMax(c + 5, b.y1);
    }
    if (b.root == big_root) {
        int32_t* const c = a.largest + 6 * m;
        atomicMin(c + 2, b.x0); atomicMin(c + 3, b.y0); atomicMax(c + 4, b.x1); atomicMax(c + 5, b.y1);
    }
}

__global__ __launch_bounds__(kCcThreads) void comp_output_kernel(const CompArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63;
    for (unsigned t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const CompTile tl = comp_tile(a, t);
        const int* const par = a.parent + tl.base;
        const unsigned long long key = a.key[tl.m];
        const int big_root = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
        if (tl.y0 == 0 && tl.col0 == 0 && tid == 0) {
            a.largest[6 * tl.m] = big_root;
            a.largest[6 * tl.m + 1] = (int)(key >> 32);
        }
        const int x = tl.col0 + tid;
        CompBox acc = {-1, 0, 0, 0, 0, 0};                      // a column's runs of one root over consecutive rows: one flush
        for (int r = 0; r < tl.n_rows; ++r) {
            const int y = tl.y0 + r;
            const int p = y * a.w + min(x, a.w - 1);
            const int v = x < a.w ? par[p] : -1;                // the root; -1 background; a root holds -2 - rank
            const bool on = v != -1;
            const int root = v < -1 ? p : v;
            const int left = __shfl_up(root, 1, 64);
            const bool head = on && (lane == 0 || left != root);
            const WaveRuns runs = {__ballot(head), __ballot(on)};
            int rank = 0, ar = 0;
            if (head) {
                rank = -2 - (v < -1 ? v : par[root]);
                if (a.keep == 1) ar = a.area[tl.base + root];
            }
            const int hl = runs.head_lane(lane);
            rank = __shfl(rank, hl, 64);
            ar = __shfl(ar, hl, 64);
            if (x < a.w) {
                if (a.labels) a.labels[tl.base + p] = on ? rank : -1;
                if (a.kept) a.kept[tl.base + p] = on && (a.keep == 1 ? ar >= a.min_area : root == big_root) ? 1 : 0;
            }
            if (head && ((unsigned)rank < (unsigned)a.max_comp || root == big_root)) {
                const int x1 = x + runs.length(lane) - 1;
                if (root == acc.root) {
                    acc.x0 = min(acc.x0, x);
                    acc.x1 = max(acc.x1, x1);
                    acc.y1 = y;
                } else {
                    comp_flush_box(a, tl.m, big_root, acc);
                    acc = {root, rank, x, y, x1, y};
                }
            }
        }
        comp_flush_box(a, tl.m, big_root, acc);
    }
}

namespace {

thread_local char components_error[256] = "";

int components_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int components_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(components_error, sizeof(components_error), fmt, ap);
    va_end(ap);
    return code;
}

bool components_sizes_ok(int n_masks, int h, int w, int max_comp)
{
    return n_masks >= 0 && n_masks <= kCcMaxMasks && h >= 1 && w >= 1 && (long long)h * w < (1ll << 31) && max_comp >= 0 &&
           max_comp <= kCcMaxComp;
}

unsigned comp_tiles_x(int w) { return (unsigned)((w + kCcTileCols - 1) / kCcTileCols); }

size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

unsigned capped(unsigned long long blocks) { return (unsigned)(blocks < kCcMaxGrid ? (blocks ? blocks : 1) : kCcMaxGrid); }

}  // namespace

}  // namespace daam

using namespace daam;

int daam_components_abi_version(void) { return DAAM_COMPONENTS_ABI_VERSION; }

const char* daam_components_last_error(void) { return components_error; }

size_t daam_mask_components_workspace(int n_masks, int h, int w, int max_comp)
{
    if (!components_sizes_ok(n_masks, h, w, max_comp)) return 0;
    const size_t pixels = (size_t)n_masks * ((size_t)h * w);
    const size_t segs = (size_t)n_masks * ((size_t)h * comp_tiles_x(w));
    return kCcHeadBytes + 2 * round8(pixels * sizeof(int)) + round8(segs * sizeof(int));
}

int daam_mask_components(const uint8_t* masks, int n_masks, int h, int w, int connectivity, int min_area, int keep, int max_comp,
                         int32_t* labels, int32_t* counts, int32_t* comps, int32_t* largest, uint8_t* kept, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    if (n_masks < 0 || n_masks > kCcMaxMasks) return components_fail(DAAM_E_INVALID, "%d masks: 0..%d", n_masks, kCcMaxMasks);
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31))
        return components_fail(DAAM_E_INVALID, "masks of %d x %d: at least 1 x 1, fewer than 2^31 pixels", h, w);
    if (connectivity != 4 && connectivity != 8) return components_fail(DAAM_E_INVALID, "connectivity %d: 4 or 8", connectivity);
    if (min_area < 0) return components_fail(DAAM_E_INVALID, "min_area %d: at least 0", min_area);
    if (keep < 0 || keep > 2) return components_fail(DAAM_E_INVALID, "keep %d: 0 none, 1 by area, 2 the largest", keep);
    if (max_comp < 0 || max_comp > kCcMaxComp) return components_fail(DAAM_E_INVALID, "max_comp %d: 0..%d", max_comp, kCcMaxComp);
    if (!masks || !counts || !largest) return components_fail(DAAM_E_INVALID, "masks, counts and largest must not be NULL");
    if ((max_comp == 0) != (comps == nullptr))
        return components_fail(DAAM_E_INVALID, "comps must be NULL exactly when max_comp is 0 (got %d)", max_comp);
    if ((keep == 0) != (kept == nullptr)) return components_fail(DAAM_E_INVALID, "kept must be NULL exactly when keep is 0 (got %d)", keep);
    if (!workspace) return components_fail(DAAM_E_INVALID, "NULL workspace");
    const size_t need = daam_mask_components_workspace(n_masks, h, w, max_comp);
    if (workspace_bytes < need)
        return components_fail(DAAM_E_INVALID, "workspace of %zu bytes: %d masks of %d x %d need %zu", workspace_bytes, n_masks, h, w, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return components_fail(DAAM_E_INVALID, "workspace is not 8-byte aligned");
    if (n_masks == 0) return 0;

    CompArgs a;
    const size_t pixels = (size_t)n_masks * ((size_t)h * w);
    unsigned char* const ws = static_cast<unsigned char*>(workspace);
    a.masks = masks;
    a.key = reinterpret_cast<unsigned long long*>(ws);
    a.parent = reinterpret_cast<int*>(ws + kCcHeadBytes);
    a.area = reinterpret_cast<int*>(ws + kCcHeadBytes + round8(pixels * sizeof(int)));
    a.seg = reinterpret_cast<int*>(ws + kCcHeadBytes + 2 * round8(pixels * sizeof(int)));
    a.labels = labels; a.counts = counts; a.comps = comps; a.largest = largest; a.kept = kept;
    a.n_masks = n_masks; a.h = h; a.w = w; a.conn8 = connectivity == 8 ? 1 : 0; a.min_area = min_area; a.keep = keep; a.max_comp = max_comp;
    a.tiles_x = comp_tiles_x(w);
    a.tiles_y = (unsigned)(((long long)h + kCcTileRows - 1) / kCcTileRows);
    // tiles_x * tiles_y <= 2^26 (w <= 256: tiles_y alone; else fewer than 2 * h * w / 8192), so all masks' tiles fit 32 bits
    a.n_tiles = (unsigned)n_masks * a.tiles_x * a.tiles_y;
    a.n_seg = (unsigned)h * a.tiles_x;                           // h (w <= 256) or < 2 * h * w / 256

    const hipStream_t s = (hipStream_t)stream;
    const dim3 block(kCcThreads), tiles(capped(a.n_tiles));
    const unsigned long long rows = (unsigned long long)n_masks * (max_comp ? max_comp : 1);
    hipLaunchKernelGGL(comp_init_kernel, dim3(capped((rows + kCcThreads - 1) / kCcThreads)), block, 0, s, a);
    hipLaunchKernelGGL(comp_local_kernel, tiles, block, 0, s, a);
    if (a.tiles_x > 1 || a.tiles_y > 1) hipLaunchKernelGGL(comp_seam_kernel, tiles, block, 0, s, a);
    hipLaunchKernelGGL(comp_flatten_kernel, tiles, block, 0, s, a);
    hipLaunchKernelGGL(comp_scan_kernel, dim3(n_masks), block, 0, s, a);
    hipLaunchKernelGGL(comp_roots_kernel, tiles, block, 0, s, a);
    hipLaunchKernelGGL(comp_output_kernel, tiles, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return components_fail((int)e, "mask_components: %s", hipGetErrorString(e));
    return 0;
}
