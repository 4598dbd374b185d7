// daam_localize (include/daam_locate.h): the bounding boxes of up to 32 word masks at up to 64 thresholds, every word's peak and
// whether it lies inside each of up to 32 truth masks, and the truth masks' boxes, from ONE pass at image resolution whatever the
// number of thresholds.  The mask of a word at tau is v > tau, so a row holds a mask pixel iff its maximum of v is
// > tau, and a column likewise; the min-max normalisation is non-decreasing in f32, so the maxima are taken on the raw resized
// values and normalised afterwards.  The value is that of daam_word_masks.hip, restated here through the same helpers of
// daam_epilogue.h (cubic_taps, enc / dec_ordered; cubic_row's expression on buffer loads; contraction off, the same operand order):
//   * locate_init_kernel    : the row / column maxima at -inf, the minima at +inf, the peak keys at 0, the truth boxes empty
//   * locate_profile_kernel : the resize -> per word the row maxima, the column maxima, the minimum and the arg-max
//   * locate_truth_kernel   : the truth bytes, 16 at a time -> the box of the set bytes of every truth mask
//   * locate_boxes_kernel   : one workgroup per word: normalise its out_h + out_w maxima, per threshold the first and last row and
//                             column above it -> boxes; the decoded peak -> peaks, peak_values, hits
// A workgroup of the profile kernel owns a tile of R output rows x 256 columns.  A lane owns 4 consecutive x, computes their taps
// once and keeps them in registers; wave k takes the rows k, k + 4, ... of the tile, whose row taps sit in an LDS table.  Words are
// the outer loop, so a word costs four column-maximum registers.  Everything is compared as enc_ordered integers: one integer
// atomicMax per (word, row, tile column) and per (word, column, tile row), one atomicMin and one 64-bit atomicMax (value, then the
// lowest row-major index) per word and tile.  No floating-point atomic: nothing depends on the grid or the order.
#include "daam_epilogue.h"
#include "../../include/daam_locate.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kLocMaxWords = 32;
constexpr int kLocMaxTruth = 32;
constexpr int kLocMaxThr = 64;
constexpr int kLocMaxSide = 128;
constexpr int kLocRun = 4;                      // consecutive x per lane
constexpr int kLocThreads = 256;
constexpr int kLocWaves = kLocThreads / 64;
constexpr int kLocTileCols = 64 * kLocRun;      // 256: the columns of a tile, one per thread when the waves' maxima are joined
constexpr int kLocMaxTileRows = 32;
constexpr int kLocTruthRows = 8;                // rows of a truth mask per wave
constexpr unsigned kLocMaxGrid = 1u << 22;      // workgroups of a launch; larger images are walked
constexpr size_t kLocHeadBytes = 512;           // peak keys [32] u64, then the minima [32] int, padded
constexpr int kLocNoPeak = kEncNegInf;          // below every finite value's encoding

struct LocateArgs {
    const float* word_maps;
    const uint8_t* truth;
    unsigned long long* key;    // [32]: ((uint32)enc_ordered(v) ^ 0x80000000) << 32 | (0xFFFFFFFF - row-major index)
    int* lo;                    // [32], enc_ordered
    int* prof;                  // [n_words][out_h + out_w], enc_ordered: the row maxima, then the column maxima
    int32_t* boxes;
    int32_t* peaks;
    float* peak_values;
    int32_t* truth_boxes;
    uint8_t* hits;
    int n_words, src_h, src_w, out_h, out_w, absolute, n_thr, n_truth;
    int tile_rows;              // R
    unsigned tiles_x, n_tiles;
    float thr[kLocMaxThr];
};

__global__ __launch_bounds__(kLocThreads) void locate_init_kernel(const LocateArgs a)
{
    const size_t n = (size_t)a.n_words * ((size_t)a.out_h + a.out_w);
    const size_t t0 = (size_t)blockIdx.x * kLocThreads + threadIdx.x;
    for (size_t i = t0; i < n; i += (size_t)gridDim.x * kLocThreads) a.prof[i] = kEncNegInf;
    if (t0 < (size_t)a.n_words) {
        a.key[t0] = 0ull;
        a.lo[t0] = kEncPosInf;
    }
    if (t0 < (size_t)a.n_truth) {
        int32_t* const b = a.truth_boxes + 4 * t0;
        b[0] = a.out_w; b[1] = a.out_h; b[2] = -1; b[3] = -1;
    }
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// cubic_row of daam_epilogue.h, the same products and sums in the same order, on buffer loads: the plane is the descriptor, the row
// a scalar byte offset (the same for the whole wave) and the lane's four columns 32-bit byte offsets.  With pointers every one of
// the 16 addresses of a pixel is a 64-bit vector add and a register pair, and the kernel takes 166 VGPRs.
__device__ __forceinline__ float locate_row(__amdgpu_buffer_rsrc_t plane, int row_bytes, const int xb[4], const float wx[4])
{
#pragma clang fp contract(off)
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(plane, xb[0], row_bytes, 0)) * wx[0] +
           __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(plane, xb[1], row_bytes, 0)) * wx[1] +
           __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(plane, xb[2], row_bytes, 0)) * wx[2] +
           __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(plane, xb[3], row_bytes, 0)) * wx[3];
}

__global__ __launch_bounds__(kLocThreads) void locate_profile_kernel(const LocateArgs a)
{
#pragma clang fp contract(off)
    __shared__ int s_iy[kLocMaxTileRows][4];            // the row taps' byte offsets into a plane
    __shared__ float s_wy[kLocMaxTileRows][4];
    __shared__ __align__(16) int s_col[2][kLocWaves][kLocTileCols];
    __shared__ int s_lo[2][kLocWaves];
    __shared__ unsigned long long s_key[2][kLocWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool identity = a.src_h == a.out_h && a.src_w == a.out_w;
    const int plane = a.src_h * a.src_w;
    const size_t n_prof = (size_t)a.out_h + a.out_w;

    for (unsigned tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const unsigned ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int y0 = (int)ty * a.tile_rows;                       // < out_h
        const int n_rows = min(a.tile_rows, a.out_h - y0);
        const int col0 = (int)tx * kLocTileCols;                    // < out_w
        const int x0 = col0 + lane * kLocRun;
        const int n_valid = min(max(a.out_w - x0, 0), kLocRun);
        if (tid < n_rows) {
            float wy[4];
            const int first = cubic_taps((float)a.src_h / (float)a.out_h, y0 + tid, wy);
            for (int t = 0; t < 4; ++t) {
                s_iy[tid][t] = min(max(first + t, 0), a.src_h - 1) * a.src_w * 4;
                s_wy[tid][t] = wy[t];
            }
        }
        int xb[kLocRun][4];                                         // the column taps, in bytes
        float wx[kLocRun][4];
        {
            const float sc = (float)a.src_w / (float)a.out_w;
#pragma unroll
            for (int k = 0; k < kLocRun; ++k) {
                const int first = cubic_taps(sc, min(x0 + k, a.out_w - 1), wx[k]);
                for (int t = 0; t < 4; ++t) xb[k][t] = min(max(first + t, 0), a.src_w - 1) * 4;
            }
        }
        __syncthreads();

#pragma unroll 1
        for (int j = 0; j < a.n_words; ++j) {
            const float* const wm = a.word_maps + (size_t)j * plane;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wm), 0, plane * 4, 0x00020000);
            int* const prof = a.prof + (size_t)j * n_prof;
            const int buf = j & 1;
            int cm[kLocRun];
#pragma unroll
            for (int k = 0; k < kLocRun; ++k) cm[k] = kEncNegInf;
            int lo = kEncPosInf, best = kLocNoPeak;
            unsigned best_at = 0;
#pragma unroll 1
            for (int r = wave; r < n_rows; r += kLocWaves) {
                const int oy = y0 + r;
                float v[kLocRun];
                if (identity) {
#pragma unroll
                    for (int k = 0; k < kLocRun; ++k) v[k] = wm[oy * a.out_w + min(x0 + k, a.out_w - 1)];
                } else {
                    // a row's taps are the same for the whole wave: scalars
                    const int iy0 = __builtin_amdgcn_readfirstlane(s_iy[r][0]), iy1 = __builtin_amdgcn_readfirstlane(s_iy[r][1]);
                    const int iy2 = __builtin_amdgcn_readfirstlane(s_iy[r][2]), iy3 = __builtin_amdgcn_readfirstlane(s_iy[r][3]);
                    const float wy0 = s_wy[r][0], wy1 = s_wy[r][1], wy2 = s_wy[r][2], wy3 = s_wy[r][3];
#pragma unroll
                    for (int k = 0; k < kLocRun; ++k) {
                        float rows[4];
                        rows[0] = locate_row(rsrc, iy0, xb[k], wx[k]);
                        rows[1] = locate_row(rsrc, iy1, xb[k], wx[k]);
                        rows[2] = locate_row(rsrc, iy2, xb[k], wx[k]);
                        rows[3] = locate_row(rsrc, iy3, xb[k], wx[k]);
                        v[k] = rows[0] * wy0 + rows[1] * wy1 + rows[2] * wy2 + rows[3] * wy3;
                    }
                }
                int rm = kEncNegInf;
#pragma unroll
                for (int k = 0; k < kLocRun; ++k)
                    if (k < n_valid) {
                        const int e = enc_ordered(v[k]);
                        cm[k] = max(cm[k], e);
                        rm = max(rm, e);
                        lo = min(lo, e);
                        if (e > best) {                             // rows and x ascend: the first of equals stays
                            best = e;
                            best_at = (unsigned)(oy * a.out_w + x0 + k);
                        }
                    }
                rm = wave_max(rm);                                  // lane 0 of every tile is a pixel: a real value
                if (lane == 0) atomicMax(prof + oy, rm);
            }
            // the tile's column maxima, minimum and peak: the four waves meet in LDS.  Two buffers, one barrier per word: a wave
            // writes buffer j & 1 again only behind the barrier of word j + 1, which every wave reaches after its reads of word j
            *reinterpret_cast<int4*>(&s_col[buf][wave][lane * kLocRun]) = make_int4(cm[0], cm[1], cm[2], cm[3]);
            unsigned long long key = ((unsigned long long)((unsigned)best ^ 0x80000000u) << 32) | (0xFFFFFFFFu - best_at);
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long other = __shfl_xor(key, off, 64);
                key = other > key ? other : key;
            }
            lo = wave_min(lo);
            if (lane == 0) {
                s_lo[buf][wave] = lo;
                s_key[buf][wave] = key;
            }
            __syncthreads();
            {
                const int m = max(max(s_col[buf][0][tid], s_col[buf][1][tid]), max(s_col[buf][2][tid], s_col[buf][3][tid]));
                if (col0 + tid < a.out_w) atomicMax(prof + a.out_h + col0 + tid, m);
            }
            if (tid == 0) {
                int l = s_lo[buf][0];
                unsigned long long k = s_key[buf][0];               // wave 0 has a row and lane 0 a pixel: a real peak
                for (int w = 1; w < kLocWaves; ++w) {
                    l = min(l, s_lo[buf][w]);
                    k = s_key[buf][w] > k ? s_key[buf][w] : k;
                }
                atomicMin(a.lo + j, l);
                atomicMax(a.key + j, k);
            }
        }
        __syncthreads();                                            // the row table and the buffers, before the next tile
    }
}

// A wave takes kLocTruthRows rows of one truth mask, a lane 16 bytes at a time at 16-byte aligned addresses: whole chunks inside the
// row through mask_bits16, the two that reach over its ends byte by byte (only the row's own bytes are read).
__global__ __launch_bounds__(kLocThreads) void locate_truth_kernel(const LocateArgs a, unsigned groups_per_mask, unsigned n_groups)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n = (size_t)a.out_h * a.out_w;
    for (unsigned grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const unsigned g = grp / groups_per_mask;
        const long long row0 = ((long long)(grp - g * groups_per_mask) * kLocWaves + wave) * kLocTruthRows;
        const uint8_t* const mask = a.truth + (size_t)g * n;
        int x0 = a.out_w, x1 = -1, y0 = a.out_h, y1 = -1;
#pragma unroll 1
        for (int rr = 0; rr < kLocTruthRows; ++rr) {
            const long long y = row0 + rr;
            if (y >= a.out_h) break;
            const uint8_t* const rp = mask + (size_t)y * a.out_w;
            const uint8_t* const re = rp + a.out_w;
            const uint8_t* c = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(rp) & ~(uintptr_t)15) + lane * 16;
#pragma unroll 1
            for (; c < re; c += 64 * 16) {
                const uint32_t bits = (c >= rp && c + 16 <= re) ? mask_bits16(*reinterpret_cast<const uint4*>(c)) : mask_bits16_edge(c, rp, re);
                if (bits) {
                    const int base = (int)(c - rp);                 // may be < 0: the set bits are bytes of the row
                    x0 = min(x0, base + __builtin_ctz(bits));
                    x1 = max(x1, base + 31 - __builtin_clz(bits));
                    y0 = min(y0, (int)y);
                    y1 = max(y1, (int)y);
                }
            }
        }
        x0 = wave_min(x0); y0 = wave_min(y0);
        x1 = wave_max(x1); y1 = wave_max(y1);
        if (lane == 0 && x1 >= 0) {
            int32_t* const b = a.truth_boxes + 4 * g;
            atomicMin(b + 0, x0);
            atomicMin(b + 1, y0);
            atomicMax(b + 2, x1);
            atomicMax(b + 3, y1);
        }
    }
}

// one workgroup per word, behind the two kernels above
__global__ __launch_bounds__(kLocThreads) void locate_boxes_kernel(const LocateArgs a)
{
#pragma clang fp contract(off)
    __shared__ int s_box[2][kLocWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const size_t n_prof = (size_t)a.out_h + a.out_w;
    int* const prof = a.prof + (size_t)j * n_prof;
    const unsigned long long key = a.key[j];
    const int hi_enc = (int)((unsigned)(key >> 32) ^ 0x80000000u);
    // the profile kernel has joined at least one pixel into the key; the clamp keeps the read of `truth` below in bounds whatever the key
    const unsigned at = min(0xFFFFFFFFu - (unsigned)key, (unsigned)a.out_h * (unsigned)a.out_w - 1u);
    const float lo = dec_ordered(a.lo[j]), hi = dec_ordered(hi_enc);

    // the maxima become the values the masks compare, in place; a thread reads back only what it wrote itself
    for (size_t i = tid; i < n_prof; i += kLocThreads) {
        float v = dec_ordered(prof[i]);
        if (!a.absolute) v = (v - lo) / (hi - lo + 1e-8f);
        prof[i] = __float_as_int(v);
    }
#pragma unroll 1
    for (int t = 0; t < a.n_thr; ++t) {
        const float thr = a.thr[t];
        int r0 = a.out_h, r1 = -1, c0 = a.out_w, c1 = -1;
        for (size_t i = tid; i < n_prof; i += kLocThreads)
            if (__int_as_float(prof[i]) > thr) {
                if (i < (size_t)a.out_h) {
                    r0 = min(r0, (int)i);
                    r1 = max(r1, (int)i);
                } else {
                    const int c = (int)(i - (size_t)a.out_h);
                    c0 = min(c0, c);
                    c1 = max(c1, c);
                }
            }
        r0 = wave_min(r0); c0 = wave_min(c0);
        r1 = wave_max(r1); c1 = wave_max(c1);
        const int buf = t & 1;                                      // two buffers, one barrier per threshold (as in the profile kernel)
        if (lane == 0) {
            s_box[buf][wave][0] = c0; s_box[buf][wave][1] = r0; s_box[buf][wave][2] = c1; s_box[buf][wave][3] = r1;
        }
        __syncthreads();
        if (tid < 4) {
            int v = s_box[buf][0][tid];
            for (int w = 1; w < kLocWaves; ++w) v = tid < 2 ? min(v, s_box[buf][w][tid]) : max(v, s_box[buf][w][tid]);
            a.boxes[((size_t)j * a.n_thr + t) * 4 + tid] = v;
        }
    }
    if (tid == 0) {
        a.peaks[2 * j] = (int)(at % (unsigned)a.out_w);
        a.peaks[2 * j + 1] = (int)(at / (unsigned)a.out_w);
        a.peak_values[3 * j] = hi;
        a.peak_values[3 * j + 1] = lo;
        a.peak_values[3 * j + 2] = hi;
    }
    if (tid < a.n_truth) a.hits[(size_t)j * a.n_truth + tid] = a.truth[(size_t)tid * a.out_h * a.out_w + at] != 0 ? 1 : 0;
}

namespace {

thread_local char locate_error[256] = "";

int locate_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int locate_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(locate_error, sizeof(locate_error), fmt, ap);
    va_end(ap);
    return code;
}

bool locate_sizes_ok(int n_words, int n_truth, int n_thr, int out_h, int out_w)
{
    return n_words >= 0 && n_words <= kLocMaxWords && n_truth >= 0 && n_truth <= kLocMaxTruth && n_words + n_truth >= 1 && n_thr >= 0 &&
           n_thr <= kLocMaxThr && out_h >= 1 && out_w >= 1 && (long long)out_h * out_w < (1ll << 31);
}

unsigned capped(unsigned long long blocks) { return (unsigned)(blocks < kLocMaxGrid ? (blocks ? blocks : 1) : kLocMaxGrid); }

}  // namespace

}  // namespace daam

using namespace daam;

int daam_locate_abi_version(void) { return DAAM_LOCATE_ABI_VERSION; }

const char* daam_locate_last_error(void) { return locate_error; }

size_t daam_localize_workspace(int n_words, int n_truth, int n_thr, int out_h, int out_w)
{
    if (!locate_sizes_ok(n_words, n_truth, n_thr, out_h, out_w)) return 0;
    const size_t prof = (size_t)n_words * ((size_t)out_h + out_w) * sizeof(int);
    return kLocHeadBytes + ((prof + 7) & ~(size_t)7);
}

int daam_localize(const float* word_maps, int n_words, int h, int w, int out_h, int out_w, int absolute, const float* thresholds, int n_thr,
                  const uint8_t* truth, int n_truth, int32_t* boxes, int32_t* peaks, float* peak_values, int32_t* truth_boxes, uint8_t* hits,
                  void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_words < 0 || n_words > kLocMaxWords) return locate_fail(DAAM_E_INVALID, "%d words: 0..%d", n_words, kLocMaxWords);
    if (n_truth < 0 || n_truth > kLocMaxTruth) return locate_fail(DAAM_E_INVALID, "%d truth masks: 0..%d", n_truth, kLocMaxTruth);
    if (n_words + n_truth < 1) return locate_fail(DAAM_E_INVALID, "neither words nor truth masks");
    if (n_thr < 0 || n_thr > kLocMaxThr) return locate_fail(DAAM_E_INVALID, "%d thresholds: 0..%d", n_thr, kLocMaxThr);
    if (h < 1 || w < 1 || h > kLocMaxSide || w > kLocMaxSide)
        return locate_fail(DAAM_E_INVALID, "word maps of %d x %d: 1 <= h, w <= %d", h, w, kLocMaxSide);
    if (out_h < 1 || out_w < 1 || (long long)out_h * out_w >= (1ll << 31))
        return locate_fail(DAAM_E_INVALID, "output of %d x %d: at least 1 x 1, fewer than 2^31 pixels", out_h, out_w);
    if (!workspace) return locate_fail(DAAM_E_INVALID, "NULL workspace");
    if ((n_words == 0) != (word_maps == nullptr) || (n_words == 0) != (peaks == nullptr) || (n_words == 0) != (peak_values == nullptr))
        return locate_fail(DAAM_E_INVALID, "word_maps, peaks and peak_values must be NULL exactly when n_words is 0 (got %d words)", n_words);
    if ((n_truth == 0) != (truth == nullptr) || (n_truth == 0) != (truth_boxes == nullptr))
        return locate_fail(DAAM_E_INVALID, "truth and truth_boxes must be NULL exactly when n_truth is 0 (got %d masks)", n_truth);
    if ((n_words * n_thr == 0) != (boxes == nullptr))
        return locate_fail(DAAM_E_INVALID, "boxes must be NULL exactly when n_words * n_thr is 0 (got %d x %d)", n_words, n_thr);
    if ((n_words * n_truth == 0) != (hits == nullptr))
        return locate_fail(DAAM_E_INVALID, "hits must be NULL exactly when n_words * n_truth is 0 (got %d x %d)", n_words, n_truth);
    if (n_thr > 0 && !thresholds) return locate_fail(DAAM_E_INVALID, "NULL thresholds with n_thr = %d", n_thr);
    for (int t = 0; t < n_thr; ++t)
        if (!std::isfinite(thresholds[t])) return locate_fail(DAAM_E_INVALID, "threshold %d is not finite", t);
    const size_t need = daam_localize_workspace(n_words, n_truth, n_thr, out_h, out_w);
    if (workspace_bytes < need)
        return locate_fail(DAAM_E_INVALID, "workspace of %zu bytes: %d words at %d x %d need %zu", workspace_bytes, n_words, out_h, out_w, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return locate_fail(DAAM_E_INVALID, "workspace is not 8-byte aligned");

    LocateArgs a;
    a.word_maps = word_maps; a.truth = truth;
    a.key = static_cast<unsigned long long*>(workspace);
    a.lo = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + kLocMaxWords * sizeof(unsigned long long));
    a.prof = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + kLocHeadBytes);
    a.boxes = boxes; a.peaks = peaks; a.peak_values = peak_values; a.truth_boxes = truth_boxes; a.hits = hits;
    a.n_words = n_words; a.src_h = h; a.src_w = w; a.out_h = out_h; a.out_w = out_w; a.absolute = absolute ? 1 : 0;
    a.n_thr = n_thr; a.n_truth = n_truth;
    a.tiles_x = (unsigned)((out_w + kLocTileCols - 1) / kLocTileCols);
    // rows of a tile: as many as 32, fewer while the image then gives fewer than 512 workgroups (the results do not depend on it)
    a.tile_rows = kLocMaxTileRows;
    while (a.tile_rows > 8 && (unsigned long long)a.tiles_x * ((out_h + a.tile_rows - 1) / a.tile_rows) < 512) a.tile_rows /= 2;
    const unsigned long long n_tiles = (unsigned long long)a.tiles_x * ((unsigned)(out_h + a.tile_rows - 1) / (unsigned)a.tile_rows);
    a.n_tiles = (unsigned)n_tiles;                                  // < 2^31 / 8 + 2^23
    for (int t = 0; t < kLocMaxThr; ++t) a.thr[t] = t < n_thr ? thresholds[t] : INFINITY;

    const hipStream_t s = (hipStream_t)stream;
    const unsigned long long cells = (unsigned long long)n_words * ((unsigned long long)out_h + out_w);
    hipLaunchKernelGGL(locate_init_kernel, dim3(capped((cells + kLocThreads - 1) / kLocThreads)), dim3(kLocThreads), 0, s, a);
    if (n_words) hipLaunchKernelGGL(locate_profile_kernel, dim3(capped(n_tiles)), dim3(kLocThreads), 0, s, a);
    if (n_truth) {
        const unsigned per_mask = (unsigned)(((long long)out_h + kLocWaves * kLocTruthRows - 1) / (kLocWaves * kLocTruthRows));
        const unsigned long long groups = (unsigned long long)per_mask * n_truth;      // <= 2^26 x 32
        hipLaunchKernelGGL(locate_truth_kernel, dim3(capped(groups)), dim3(kLocThreads), 0, s, a, per_mask, (unsigned)groups);
    }
    if (n_words) hipLaunchKernelGGL(locate_boxes_kernel, dim3(n_words), dim3(kLocThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return locate_fail((int)e, "localize: %s", hipGetErrorString(e));
    return 0;
}
