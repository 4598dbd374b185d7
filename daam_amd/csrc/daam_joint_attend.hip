// libdaam_jointattend.so (include/daam_joint_attend.h): the joint attention of an MMDiT block with the tap's statistics as a
// by-product of its key walk, and the text columns from given statistics.  The MFMA wrapper, acc_row, the normalise-add
// (add_prob) and the weighted store are RESTATED here from the header that the self-affinity and the joint tap share, as
// daam_joint_affinity.hip restates them: that header's readers are pinned to those two libraries, so this file reads nothing of csrc/.
// add_prob must stay the expression of joint_text_kernel in daam_joint_tap.hip, term for term.
//   * joint_attend_kernel<DT, D>      : joint_stats_kernel's walk, extended.  A workgroup of four waves owns 128 query rows of one
//                                       slice and one kind (image or text), 32 per wave, held as the MFMA B operand for the whole
//                                       walk.  It walks first the text keys and then the image keys in tiles of KT = 4096 / D keys
//                                       (64 with d = 64, 32 with d = 128: K and V, two buffers deep each, stay under 64 KB); the next
//                                       tile's global loads are issued before the current tile's MFMAs and land in the other buffers
//                                       after them, one barrier per tile.  K Q^T with mfma_f32_32x32x16 puts 32 keys on the
//                                       accumulator's rows and a query on the lane.  Per 32-key step the two lane halves exchange
//                                       their maxima (one shuffle), so the running maximum m is the row's; the sum l stays per half
//                                       until the end.  p = exp2(fma(raw, c, -(m c))) is rounded to the input dtype, registers
//                                       8 s .. 8 s + 7 as the B fragment of k-step s of O^T += V^T P^T: no lane movement, no LDS.  The
//                                       V^T fragment enumerates the keys as the accumulator rows do -- element j of lane half h is key
//                                       16 s + 8 (j >> 2) + 4 h + (j & 3) -- with two ds_read_b64_tr_b16 of 4 keys x 16 channels each
//                                       from a row-major V tile whose rows are D + 32 elements apart (the 4 rows of a read land 16
//                                       banks apart: no conflict by the bank rule; no counter was read).  The output accumulators
//                                       (D / 32 blocks of 16 registers, channels on the rows) are rescaled by exp2 of the maximum's
//                                       move, lane-local.  Padded keys are -inf in a partial step only; padded K and V rows are zero
//                                       in LDS.  Epilogue: o = acc (1 / l), one rounding, 8-byte stores of 4 channels; image blocks
//                                       write (-(m c), 1 / l).  With bf16 the fragment of p carries 2^-15 and the epilogue's 1 / l
//                                       carries 2^15 (Round16), so that the accumulator stays inside f32 for V up to the dtype's
//                                       largest finite value.
//   * joint_attend_text_kernel<DT, D> : joint_text_kernel of daam_joint_tap.hip, restated line for line.
// No atomics, no dependence on the grid: two runs give the same bits.
#include "../../include/daam_joint_attend.h"
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace daam {

constexpr int kJfMaxP = 16384;                      // image rows (queries and keys) of a slice
constexpr int kJfMaxT = 512;                        // text rows
constexpr int kJfMaxSlices = 4096;                  // batch x heads
constexpr int kJfThreads = 256;
constexpr int kJfRows = 128;                        // query rows of a block; rows of a slice's statistics are padded to whole blocks
constexpr int kJfTextTile = 64;                     // text rows of an output tile of the text kernel

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bfloat8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef __bf16 bfloat4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));

template <int DT> struct Mma32;
template <> struct Mma32<DAAM_F16> {
    static __device__ __forceinline__ floatx16 run(const uint4& a, const uint4& b, const floatx16& c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
    }
};
template <> struct Mma32<DAAM_BF16> {
    static __device__ __forceinline__ floatx16 run(const uint4& a, const uint4& b, const floatx16& c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bfloat8, a), __builtin_bit_cast(bfloat8, b), c, 0, 0, 0);
    }
};

// The row of a 32 x 32 accumulator block that register `reg` of lane half `half` holds (the column is lane & 31).
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// acc + the probability of a raw dot product under its row's statistics st = (-(m c), 1 / l).
__device__ __forceinline__ float add_prob(float x, float c, const float2& st, float acc)
{
    return __fmaf_rn(__builtin_amdgcn_exp2f(__fmaf_rn(x, c, st.x)), st.y, acc);
}

// The one read-modify-write of an element of sums at the end of the text kernel.
__device__ __forceinline__ void store_weighted(float* out, float weight, float acc, int accumulate)
{
    *out = __fmaf_rn(weight, acc, accumulate ? *out : 0.f);
}

// Eight / four f32 rounded to the input dtype (round to nearest even), as the bits of an MFMA fragment / of an 8-byte store.
template <int DT> struct Round16;
template <> struct Round16<DAAM_F16> {
    static constexpr float kFold = 1.0f, kUnfold = 1.0f;
    static __device__ __forceinline__ uint4 eight(const floatx16& p, int s)
    {
        half8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (_Float16)p[8 * s + j];
        return __builtin_bit_cast(uint4, h);
    }
    static __device__ __forceinline__ uint2 four(float a, float b, float c, float d)
    {
        const half4 h = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
        return __builtin_bit_cast(uint2, h);
    }
};
// bf16 shares f32's exponent range, and the output accumulator holds sum e v BEFORE the division by l <= T + P < 2^15: with |v| near the
// largest finite value it would leave f32.  The bf16 fragment of e therefore carries a factor 2^-15 (exact but for e < 2^-111, which
// falls below the normal range), and the epilogue's 1 / l carries 2^15: sum (2^-15 e) v <= 2^-15 l max|v| stays finite.
template <> struct Round16<DAAM_BF16> {
    static constexpr float kFold = 0x1p-15f, kUnfold = 0x1p15f;
    static __device__ __forceinline__ uint4 eight(const floatx16& p, int s)
    {
        bfloat8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (__bf16)(p[8 * s + j] * kFold);
        return __builtin_bit_cast(uint4, h);
    }
    static __device__ __forceinline__ uint2 four(float a, float b, float c, float d)
    {
        const bfloat4 h = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
        return __builtin_bit_cast(uint2, h);
    }
};

struct JfStrides {
    long long sb, sh, sp;                           // batch, head, row, in elements
};

struct JfGeom {
    int heads, P, T;
    int p_pad;                                      // P rounded up to whole blocks: the row count of a slice's statistics
    int blocks_img, blocks_txt;                     // query blocks of a slice, the image blocks first
    JfStrides qi, ki, vi, qt, kt, vt, oi, ot;
};

// A tile of ROWS rows x D elements, rows row0 .. of a [limit][D] matrix with row stride `stride`, as 16-byte chunks: chunk c of the
// tile (row c / CH, chunk c % CH of the row) is thread c % 256's element c / 256 of `stage`.  Rows >= limit are zero.
template <int D, int ROWS>
__device__ __forceinline__ void jf_fetch(uint4 (&stage)[ROWS * (D / 8) / kJfThreads], const uint16_t* __restrict__ base, long long stride,
                                         int row0, int limit)
{
    constexpr int CH = D / 8;
#pragma unroll
    for (int e = 0; e < ROWS * CH / kJfThreads; ++e) {
        const int c = threadIdx.x + e * kJfThreads;
        const int r = c / CH, ch = c - r * CH, row = row0 + r;
        stage[e] = make_uint4(0, 0, 0, 0);
        if (row < limit) stage[e] = *reinterpret_cast<const uint4*>(base + (long long)row * stride + ch * 8);
    }
}

// ... into LDS, D / 8 + PAD chunks to a row.
template <int D, int ROWS, int PAD>
__device__ __forceinline__ void jf_commit(uint4* __restrict__ lds, const uint4 (&stage)[ROWS * (D / 8) / kJfThreads])
{
    constexpr int CH = D / 8;
#pragma unroll
    for (int e = 0; e < ROWS * CH / kJfThreads; ++e) {
        const int c = threadIdx.x + e * kJfThreads;
        const int r = c / CH, ch = c - r * CH;
        lds[r * (CH + PAD) + ch] = stage[e];
    }
}

constexpr int kJfKPad = 1;                          // chunks of padding of a K row in LDS: row reads of 16 bytes
constexpr int kJfVPad = 4;                          // ... of a V row: the four rows of a transposed read land 16 banks apart

template <int DT, int D>
__global__ __launch_bounds__(kJfThreads) void joint_attend_kernel(const uint16_t* __restrict__ q_img, const uint16_t* __restrict__ k_img,
                                                                  const uint16_t* __restrict__ v_img, const uint16_t* __restrict__ q_txt,
                                                                  const uint16_t* __restrict__ k_txt, const uint16_t* __restrict__ v_txt,
                                                                  uint16_t* __restrict__ out_img, uint16_t* __restrict__ out_txt,
                                                                  float2* __restrict__ stats, JfGeom g, float c)
{
    constexpr int CH = D / 8, KK = D / 16, CB = D / 32, KT = 4096 / D;
    constexpr int KSTR = CH + kJfKPad, VSTR = CH + kJfVPad, STAGE = KT * CH / kJfThreads;
    static_assert(KT % 32 == 0 && STAGE >= 1, "a tile is whole 32-key steps and at least a chunk per thread");
    __shared__ uint4 lds_k[2][KT * KSTR];
    __shared__ uint4 lds_v[2][KT * VSTR];
    const int per_slice = g.blocks_img + g.blocks_txt;
    const int s = blockIdx.x / per_slice, blk = blockIdx.x - s * per_slice;
    const bool text_rows = blk >= g.blocks_img;
    const int i0 = (text_rows ? blk - g.blocks_img : blk) * kJfRows, n_rows = text_rows ? g.T : g.P;
    const int b = s / g.heads, hd = s - b * g.heads;
    const JfStrides qst = text_rows ? g.qt : g.qi, ost = text_rows ? g.ot : g.oi;
    const uint16_t* qs = (text_rows ? q_txt : q_img) + b * qst.sb + hd * qst.sh;
    const uint16_t* kts = k_txt + b * g.kt.sb + hd * g.kt.sh;
    const uint16_t* kis = k_img + b * g.ki.sb + hd * g.ki.sh;
    const uint16_t* vts = v_txt + b * g.vt.sb + hd * g.vt.sh;
    const uint16_t* vis = v_img + b * g.vi.sb + hd * g.vi.sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;

    // the wave's 32 queries as the B operand: lane (r, half) holds Q[row r][16 kk + 8 half ..], kept for the whole walk
    const int qrow = i0 + wave * 32 + r;
    uint4 qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        qf[kk] = make_uint4(0, 0, 0, 0);
        if (qrow < n_rows) qf[kk] = *reinterpret_cast<const uint4*>(qs + (long long)qrow * qst.sp + kk * 16 + half * 8);
    }

    // this lane's part of a transposed read of V, in 8-byte units: lane 4 q + p of a group of 16 gives row q, columns 4 p .. 4 p + 3 of a
    // block of 4 keys x 16 channels and receives the 4 keys of column lane & 15; the group's block is keys 4 half .., channels
    // 16 ((lane >> 4) & 1) .. of a 32-channel block
    const int v_lane = (((lane >> 2) & 3) + 4 * half) * (VSTR * 2) + 4 * ((lane >> 4) & 1) + (lane & 3);

    // the walk: tiles 0 .. n_txt - 1 are text keys, the rest image keys
    const int n_txt = (g.T + KT - 1) / KT, n_all = n_txt + (g.P + KT - 1) / KT;
    uint4 stage_k[STAGE], stage_v[STAGE];
    jf_fetch<D, KT>(stage_k, kts, g.kt.sp, 0, g.T);
    jf_fetch<D, KT>(stage_v, vts, g.vt.sp, 0, g.T);
    jf_commit<D, KT, kJfKPad>(lds_k[0], stage_k);
    jf_commit<D, KT, kJfVPad>(lds_v[0], stage_v);
    __syncthreads();

    floatx16 acc[CB];                               // O^T: block cb holds channels 32 cb + acc_row(reg, half) of query r
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[cb] = floatx16{0};
    float m = -INFINITY, negm = 0.f;                // of the row: both lane halves hold the same
    float l = 0.f;                                  // of this lane's half of the keys
    for (int t = 0; t < n_all; ++t) {
        const bool txt = t < n_txt;
        const int j0 = (txt ? t : t - n_txt) * KT, limit = txt ? g.T : g.P;
        if (t + 1 < n_all) {                        // the next tile's loads are in flight under this tile's MFMAs
            const bool ntxt = t + 1 < n_txt;
            const int nrow0 = (ntxt ? t + 1 : t + 1 - n_txt) * KT, nlimit = ntxt ? g.T : g.P;
            jf_fetch<D, KT>(stage_k, ntxt ? kts : kis, ntxt ? g.kt.sp : g.ki.sp, nrow0, nlimit);
            jf_fetch<D, KT>(stage_v, ntxt ? vts : vis, ntxt ? g.vt.sp : g.vi.sp, nrow0, nlimit);
        }
        const uint4* cur_k = lds_k[t & 1];
        const __attribute__((address_space(3))) short4v* cur_v =
            (const __attribute__((address_space(3))) short4v*)(lds_v[t & 1]) + v_lane;
#pragma unroll
        for (int sub = 0; sub < KT / 32; ++sub) {
            const int k0 = j0 + sub * 32;
            if (k0 >= limit) break;                 // no key at all in this step (uniform over the workgroup)
            floatx16 x = {0};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) x = Mma32<DT>::run(cur_k[(sub * 32 + r) * KSTR + kk * 2 + half], qf[kk], x);
            if (k0 + 32 > limit) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (k0 + acc_row(reg, half) >= limit) x[reg] = -INFINITY;
            }
            float top = x[0];
#pragma unroll
            for (int reg = 1; reg < 16; ++reg) top = fmaxf(top, x[reg]);
            top = fmaxf(top, __shfl_xor(top, 32));  // key k0 is real and sits in the lower half: finite
            const float m_new = fmaxf(m, top);
            const float negm_new = -(m_new * c);
            const float carry = m > -INFINITY ? __builtin_amdgcn_exp2f(negm_new - negm) : 0.f;
            float part = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                x[reg] = __builtin_amdgcn_exp2f(__fmaf_rn(x[reg], c, negm_new));
                part += x[reg];
            }
            l = l * carry + part;
            m = m_new;
            negm = negm_new;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) acc[cb][reg] *= carry;
            // O^T += V^T P^T: two k-steps of 16 keys; the A fragment's elements 0 .. 3 are keys 16 ks + 4 half + (0 .. 3), 4 .. 7 those
            // 8 further on -- the order of the accumulator rows that Round16::eight packs
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 pf = Round16<DT>::eight(x, ks);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const int at = (sub * 32 + ks * 16) * (VSTR * 2) + cb * 8;
                    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        const_cast<__attribute__((address_space(3))) short4v*>(cur_v + at));
                    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        const_cast<__attribute__((address_space(3))) short4v*>(cur_v + at + 8 * (VSTR * 2)));
                    const short8v vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[cb] = Mma32<DT>::run(__builtin_bit_cast(uint4, vf), pf, acc[cb]);
                }
            }
        }
        // buffers (t + 1) & 1 were last read in step t - 1, which every wave left through the barrier below
        if (t + 1 < n_all) {
            jf_commit<D, KT, kJfKPad>(lds_k[(t + 1) & 1], stage_k);
            jf_commit<D, KT, kJfVPad>(lds_v[(t + 1) & 1], stage_v);
        }
        __syncthreads();
    }
    // the two halves of the keys share m; the lower half's sum first
    const float l_o = __shfl_xor(l, 32);
    const float rinv = 1.0f / (half ? l_o + l : l + l_o);
    if (!text_rows && stats != nullptr && half == 0) stats[(size_t)s * g.p_pad + qrow] = make_float2(negm, rinv);
    const float rout = rinv * Round16<DT>::kUnfold; // exact: 1 / l <= 1
    if (qrow < n_rows) {
        uint16_t* const orow = (text_rows ? out_txt : out_img) + b * ost.sb + hd * ost.sh + (long long)qrow * ost.sp;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int grp = 0; grp < 4; ++grp)
                *reinterpret_cast<uint2*>(orow + cb * 32 + 8 * grp + 4 * half) =
                    Round16<DT>::four(acc[cb][4 * grp] * rout, acc[cb][4 * grp + 1] * rout, acc[cb][4 * grp + 2] * rout,
                                      acc[cb][4 * grp + 3] * rout);
    }
}

struct JtGeom {
    int heads, P, T, n_slices;
    int p_pad;
    int plane_step;                                 // slices between two of a plane: 1 (one plane) or heads (a plane per head)
    long long plane_stride;                         // floats between two planes
    long long q_sb, q_sh, q_sp, kt_sb, kt_sh, kt_sp;
};

template <int DT, int D>
__global__ __launch_bounds__(kJfThreads) void joint_attend_text_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_txt,
                                                                       const float2* __restrict__ stats, float* __restrict__ sums, JtGeom g,
                                                                       float c, float weight, int accumulate)
{
    constexpr int CH = D / 8, KK = D / 16;
    __shared__ uint4 lds_q[kJfRows * (CH + 1)];
    __shared__ uint4 lds_k[kJfTextTile * (CH + 1)];
    const int cell_tiles = g.p_pad / kJfRows, txt_tiles = (g.T + kJfTextTile - 1) / kJfTextTile;
    const int plane = blockIdx.x / (cell_tiles * txt_tiles), rest = blockIdx.x - plane * (cell_tiles * txt_tiles);
    const int tt = rest / cell_tiles, ti = rest - tt * cell_tiles;
    const int t0 = tt * kJfTextTile, i0 = ti * kJfRows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
    const int cell = i0 + wave * 32 + r;            // this lane's column; < p_pad

    floatx16 acc[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[mi] = floatx16{0};

    // the slices of this plane, ascending: every slice (plane 0 of one), or those of head `plane`
    for (int s = plane; s < g.n_slices; s += g.plane_step) {
        const int b = s / g.heads, hd = s - b * g.heads;
        uint4 stage_q[kJfRows * CH / kJfThreads], stage_k[kJfTextTile * CH / kJfThreads];
        jf_fetch<D, kJfRows>(stage_q, q + b * g.q_sb + hd * g.q_sh, g.q_sp, i0, g.P);
        jf_fetch<D, kJfTextTile>(stage_k, k_txt + b * g.kt_sb + hd * g.kt_sh, g.kt_sp, t0, g.T);
        const float2 st = stats[(size_t)s * g.p_pad + cell];
        __syncthreads();                            // the previous slice's reads are done
        jf_commit<D, kJfRows, 1>(lds_q, stage_q);
        jf_commit<D, kJfTextTile, 1>(lds_k, stage_k);
        __syncthreads();
        floatx16 x[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) x[mi] = floatx16{0};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const uint4 bq = lds_q[(wave * 32 + r) * (CH + 1) + kk * 2 + half];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) x[mi] = Mma32<DT>::run(lds_k[(mi * 32 + r) * (CH + 1) + kk * 2 + half], bq, x[mi]);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc[mi][reg] = add_prob(x[mi][reg], c, st, acc[mi][reg]);
    }

    float* const out_plane = sums + plane * g.plane_stride;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int tok = t0 + mi * 32 + acc_row(reg, half);
            if (tok < g.T && cell < g.P) store_weighted(out_plane + (size_t)tok * g.P + cell, weight, acc[mi][reg], accumulate);
        }
}

namespace {

thread_local char last_error[256] = "";

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
    return DAAM_E_INVALID;
}

int pad_rows(int n) { return (n + kJfRows - 1) / kJfRows * kJfRows; }

// Bytes of the statistics of batch x heads slices of P rows; 0 when out of range.
size_t stats_bytes_of(int batch, int heads, int P)
{
    if (batch < 1 || heads < 1 || (long long)batch * heads > kJfMaxSlices || P < 1 || P > kJfMaxP) return 0;
    return sizeof(float2) * (size_t)batch * heads * pad_rows(P);
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The checks both entry points share, in the order they report them.
int check_common(const char* who, int in_dtype, int batch, int heads, int P, int T, int d, float scale)
{
    if (in_dtype != DAAM_F16 && in_dtype != DAAM_BF16) return fail("%s: dtype %d: fp16 (DAAM_F16) or bf16 (DAAM_BF16)", who, in_dtype);
    if (batch < 1 || heads < 1 || (long long)batch * heads > kJfMaxSlices)
        return fail("%s: batch %d x heads %d: each >= 1 and no more than %d slices", who, batch, heads, kJfMaxSlices);
    if (P < 1 || P > kJfMaxP) return fail("%s: P %d: 1..%d", who, P, kJfMaxP);
    if (T < 1 || T > kJfMaxT) return fail("%s: T %d: 1..%d", who, T, kJfMaxT);
    if (d != 64 && d != 128) return fail("%s: head dim %d: 64 or 128", who, d);
    if (!std::isfinite(scale) || !(scale > 0.f)) return fail("%s: scale %g: a finite number above 0", who, (double)scale);
    return 0;
}

int check_strides(const char* who, const char* name, const int64_t* st, int d)
{
    for (int i = 0; i < 3; ++i)
        if (st[i] < 0 || (st[i] & 7) || st[i] > ((int64_t)1 << 40))
            return fail("%s: %s stride %lld: >= 0 and whole 16-byte rows (8 elements)", who, name, (long long)st[i]);
    if (st[2] < d) return fail("%s: %s row stride %lld below the head dim %d", who, name, (long long)st[2], d);
    return 0;
}

// Bytes from a tensor's first to past its last element.
size_t extent_bytes(const int64_t* st, int batch, int heads, int rows, int d)
{
    return 2 * ((size_t)(batch - 1) * (size_t)st[0] + (size_t)(heads - 1) * (size_t)st[1] + (size_t)(rows - 1) * (size_t)st[2] + (size_t)d);
}

JfStrides strides_of(const int64_t* st) { return JfStrides{(long long)st[0], (long long)st[1], (long long)st[2]}; }

int launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fail("%s: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

template <int DT, int D>
void launch_forward(hipStream_t s, const void* const* in, void* out_img, void* out_txt, float2* stats, const JfGeom& g, int slices, float c)
{
    const unsigned blocks = (unsigned)(g.blocks_img + g.blocks_txt) * (unsigned)slices;
    hipLaunchKernelGGL((joint_attend_kernel<DT, D>), dim3(blocks), dim3(kJfThreads), 0, s, static_cast<const uint16_t*>(in[0]),
                       static_cast<const uint16_t*>(in[1]), static_cast<const uint16_t*>(in[2]), static_cast<const uint16_t*>(in[3]),
                       static_cast<const uint16_t*>(in[4]), static_cast<const uint16_t*>(in[5]), static_cast<uint16_t*>(out_img),
                       static_cast<uint16_t*>(out_txt), stats, g, c);
}

template <int DT, int D>
void launch_text(hipStream_t s, const void* q, const void* k_txt, const float2* stats, float* sums, const JtGeom& g, int planes, float c,
                 float weight, int accumulate)
{
    const unsigned tiles = (unsigned)(g.p_pad / kJfRows) * (unsigned)((g.T + kJfTextTile - 1) / kJfTextTile) * (unsigned)planes;
    hipLaunchKernelGGL((joint_attend_text_kernel<DT, D>), dim3(tiles), dim3(kJfThreads), 0, s, static_cast<const uint16_t*>(q),
                       static_cast<const uint16_t*>(k_txt), stats, sums, g, c, weight, accumulate);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_joint_attend_abi_version(void) { return DAAM_JOINT_ATTEND_ABI_VERSION; }

const char* daam_joint_attend_last_error(void) { return last_error; }

size_t daam_joint_attend_stats_bytes(int batch, int heads, int P) { return stats_bytes_of(batch, heads, P); }

int daam_joint_attend_forward(const void* q_img, const void* k_img, const void* v_img, const void* q_txt, const void* k_txt,
                              const void* v_txt, void* out_img, void* out_txt, int in_dtype, int batch, int heads, int P, int T, int d,
                              const int64_t* img_strides, const int64_t* txt_strides, const int64_t* out_strides, float scale, void* stats,
                              size_t stats_bytes, void* stream)
{
    const char* who = "joint_attend_forward";
    if (const int rc = check_common(who, in_dtype, batch, heads, P, T, d, scale)) return rc;
    if (!q_img || !k_img || !v_img || !q_txt || !k_txt || !v_txt || !out_img || !out_txt || !img_strides || !txt_strides || !out_strides)
        return fail("%s: the six inputs, the two outputs and the three stride arrays must not be NULL", who);
    const void* const in[6] = {q_img, k_img, v_img, q_txt, k_txt, v_txt};
    static const char* const names[8] = {"q_img", "k_img", "v_img", "q_txt", "k_txt", "v_txt", "out_img", "out_txt"};
    const void* const all[8] = {q_img, k_img, v_img, q_txt, k_txt, v_txt, out_img, out_txt};
    const int64_t* const st[8] = {img_strides, img_strides + 3, img_strides + 6, txt_strides, txt_strides + 3, txt_strides + 6,
                                  out_strides, out_strides + 3};
    const int rows[8] = {P, P, P, T, T, T, P, T};
    for (int i = 0; i < 8; ++i)
        if (reinterpret_cast<uintptr_t>(all[i]) & 15) return fail("%s: %s must be 16-byte aligned", who, names[i]);
    for (int i = 0; i < 8; ++i)
        if (const int rc = check_strides(who, names[i], st[i], d)) return rc;
    for (int i = 6; i < 8; ++i) {
        // no two rows of an output share an element: the rows of a head lie inside its stride, or the heads of a row inside the row
        // stride; the batch entries lie apart by what one of them spans
        const int64_t sb = st[i][0], sh = st[i][1], sp = st[i][2], n = rows[i];
        const bool rows_in_head = sh >= (n - 1) * sp + d, heads_in_row = sh >= d && sp >= (int64_t)(heads - 1) * sh + d;
        if (heads > 1 && !rows_in_head && !heads_in_row)
            return fail("%s: %s strides head %lld / row %lld: rows of two heads would share elements", who, names[i], (long long)sh, (long long)sp);
        if (batch > 1 && sb < (int64_t)(heads - 1) * sh + (n - 1) * sp + d)
            return fail("%s: %s batch stride %lld: two batch entries would share elements", who, names[i], (long long)sb);
        for (int j = 0; j < 6; ++j)
            if (overlap(all[i], extent_bytes(st[i], batch, heads, rows[i], d), all[j], extent_bytes(st[j], batch, heads, rows[j], d)))
                return fail("%s: %s overlaps %s", who, names[i], names[j]);
    }
    if (overlap(out_img, extent_bytes(st[6], batch, heads, P, d), out_txt, extent_bytes(st[7], batch, heads, T, d)))
        return fail("%s: out_img overlaps out_txt", who);
    if (stats) {
        if (reinterpret_cast<uintptr_t>(stats) & 7) return fail("%s: stats must be 8-byte aligned", who);
        const size_t need = stats_bytes_of(batch, heads, P);
        if (stats_bytes < need) return fail("%s: stats of %zu bytes: %d slices x %d rows take %zu", who, stats_bytes, batch * heads, P, need);
        for (int i = 0; i < 8; ++i)
            if (overlap(stats, stats_bytes, all[i], extent_bytes(st[i], batch, heads, rows[i], d)))
                return fail("%s: stats overlap %s", who, names[i]);
    }

    JfGeom g;
    g.heads = heads; g.P = P; g.T = T; g.p_pad = pad_rows(P);
    g.blocks_img = g.p_pad / kJfRows; g.blocks_txt = (T + kJfRows - 1) / kJfRows;
    g.qi = strides_of(st[0]); g.ki = strides_of(st[1]); g.vi = strides_of(st[2]);
    g.qt = strides_of(st[3]); g.kt = strides_of(st[4]); g.vt = strides_of(st[5]);
    g.oi = strides_of(st[6]); g.ot = strides_of(st[7]);
    const float c = (float)((double)scale * 1.4426950408889634);        // scale log2(e), rounded once: the c of the statistics
    const hipStream_t s = (hipStream_t)stream;
    float2* const sp = static_cast<float2*>(stats);
    const int slices = batch * heads;
    if (in_dtype == DAAM_F16) {
        if (d == 64) launch_forward<DAAM_F16, 64>(s, in, out_img, out_txt, sp, g, slices, c);
        else launch_forward<DAAM_F16, 128>(s, in, out_img, out_txt, sp, g, slices, c);
    } else {
        if (d == 64) launch_forward<DAAM_BF16, 64>(s, in, out_img, out_txt, sp, g, slices, c);
        else launch_forward<DAAM_BF16, 128>(s, in, out_img, out_txt, sp, g, slices, c);
    }
    return launched(who);
}

int daam_joint_attend_text(const void* q_img, const void* k_txt, const void* stats, size_t stats_bytes, int in_dtype, int batch, int heads,
                           int P, int T, int d, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p, int64_t kt_stride_b,
                           int64_t kt_stride_h, int64_t kt_stride_t, float scale, float weight, int accumulate, float* sums,
                           int64_t sums_stride_h, void* stream)
{
    const char* who = "joint_attend_text";
    if (const int rc = check_common(who, in_dtype, batch, heads, P, T, d, scale)) return rc;
    if (!std::isfinite(weight)) return fail("%s: weight %g: a finite number", who, (double)weight);
    if (!q_img || !k_txt || !stats || !sums) return fail("%s: q_img, k_txt, stats and sums must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(q_img) | reinterpret_cast<uintptr_t>(k_txt)) & 15)
        return fail("%s: q_img and k_txt must be 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(stats) & 7) return fail("%s: stats must be 8-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(sums) & 3) return fail("%s: sums must be 4-byte aligned", who);
    const int64_t qst[3] = {q_stride_b, q_stride_h, q_stride_p}, kst[3] = {kt_stride_b, kt_stride_h, kt_stride_t};
    if (const int rc = check_strides(who, "q_img", qst, d)) return rc;
    if (const int rc = check_strides(who, "k_txt", kst, d)) return rc;
    const int64_t plane = (int64_t)T * P;
    if (sums_stride_h != 0 && sums_stride_h < plane)
        return fail("%s: sums_stride_h %lld: 0 (one plane) or >= T * P = %lld", who, (long long)sums_stride_h, (long long)plane);
    if (sums_stride_h > ((int64_t)1 << 40)) return fail("%s: sums_stride_h %lld is out of range", who, (long long)sums_stride_h);
    const int planes = sums_stride_h ? heads : 1;
    const size_t sums_bytes = sizeof(float) * ((size_t)(planes - 1) * (size_t)sums_stride_h + (size_t)plane);
    const size_t need = stats_bytes_of(batch, heads, P);
    if (stats_bytes < need) return fail("%s: stats of %zu bytes: %d slices x %d rows take %zu", who, stats_bytes, batch * heads, P, need);
    if (overlap(sums, sums_bytes, stats, stats_bytes)) return fail("%s: stats overlap sums", who);

    JtGeom g;
    g.heads = heads; g.P = P; g.T = T; g.n_slices = batch * heads; g.p_pad = pad_rows(P);
    g.plane_step = sums_stride_h ? heads : 1; g.plane_stride = sums_stride_h;
    g.q_sb = q_stride_b; g.q_sh = q_stride_h; g.q_sp = q_stride_p;
    g.kt_sb = kt_stride_b; g.kt_sh = kt_stride_h; g.kt_sp = kt_stride_t;
    const float c = (float)((double)scale * 1.4426950408889634);
    const hipStream_t s = (hipStream_t)stream;
    const float2* const st = static_cast<const float2*>(stats);
    const int acc = accumulate != 0;
    if (in_dtype == DAAM_F16) {
        if (d == 64) launch_text<DAAM_F16, 64>(s, q_img, k_txt, st, sums, g, planes, c, weight, acc);
        else launch_text<DAAM_F16, 128>(s, q_img, k_txt, st, sums, g, planes, c, weight, acc);
    } else {
        if (d == 64) launch_text<DAAM_BF16, 64>(s, q_img, k_txt, st, sums, g, planes, c, weight, acc);
        else launch_text<DAAM_BF16, 128>(s, q_img, k_txt, st, sums, g, planes, c, weight, acc);
    }
    return launched(who);
}
