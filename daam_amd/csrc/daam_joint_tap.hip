// daam_joint_tap_accumulate (include/daam_joint_tap.h): the text columns of the joint softmax of an MMDiT attention call -- image
// queries over text AND image keys -- summed over slices into heat-map planes f32 [T][P].  Row statistics first, then a second
// kernel that recomputes a tile and normalises it.  The MFMA wrapper, acc_row, the normalise-add, the weighted store and the common host
// checks are those of daam_rowsoftmax32.h; the online step and the merge of the lane halves stand here and, the same text, in
// daam_self_affinity.hip (as a function either of them reschedules the statistics kernels): a fix to one is a fix to both.
//   * joint_stats_kernel<DT, D>  : a workgroup of four waves owns 128 query rows of one slice, 32 per wave, and walks first the text
//                                  keys and then the image keys in tiles of 64 that go through LDS, two buffers deep: the next
//                                  tile's global loads are issued before the current tile's MFMAs and land in the other buffer
//                                  after them, one barrier per tile.  It computes K Q^T with mfma_f32_32x32x16 (keys on the
//                                  accumulator's rows, the wave's queries on the lanes), so a row's maximum and sum are reductions
//                                  over a lane's registers plus one exchange between the two lane halves at the very end.  Online:
//                                  per lane the running maximum m of the raw dot products and l = sum exp2(fma(raw, c, -(m c))),
//                                  c = f32(scale log2 e); padded keys count as -inf, a 32-key step with no key at all is skipped.
//                                  It writes (-(m c), 1 / l) per row.
//   * joint_text_kernel<DT, D>   : a workgroup owns a 64 x 128 tile (text rows x cells) of one output plane, a wave 64 x 32 (2 MFMA
//                                  blocks, text keys on the rows, cells on the lanes so that stores run along the cells).  It loops
//                                  over the slices of its plane in ascending order, recomputes the tile's dot products from k_txt and
//                                  Q tiles in LDS and adds exp2(fma(raw, c, -(m c))) * (1 / l) with one fma into 32 accumulators per
//                                  lane that stay in registers across the whole loop; one read-modify-write of sums at the end.
// Rows past T / Pk / P are zero-filled in LDS, masked in the statistics and not stored in the epilogue.
// No atomics, no dependence on the grid: two runs give the same bits.
#include "../../include/daam_joint_tap.h"
#include "daam_rowsoftmax32.h"

namespace daam {

constexpr int kJtMaxT = 512;
constexpr int kJtThreads = 256;
constexpr int kJtRows = kRowTile;                   // query rows of a statistics block, cells of an output tile
constexpr int kJtKeyTile = 64;                      // keys per step of the statistics walk, text rows of an output tile

struct JtGeom {
    int heads, P, T, Pk, n_slices;
    int p_pad;                                      // P rounded up to whole blocks: the row count of a slice's statistics
    int plane_step;                                 // slices between two of a plane: 1 (one plane) or heads (a plane per head)
    long long plane_stride;                         // floats between two planes
    long long q_sb, q_sh, q_sp, kt_sb, kt_sh, kt_sp, ki_sb, ki_sh, ki_sp;
};

// A tile of ROWS rows x D elements, rows row0 .. of a [limit][D] matrix with row stride `stride`, as 16-byte chunks: chunk c of the
// tile (row c / CH, chunk c % CH of the row) is thread c % 256's element c / 256 of `stage`.  Rows >= limit are zero.
template <int D, int ROWS>
__device__ __forceinline__ void jt_fetch(uint4 (&stage)[ROWS * (D / 8) / kJtThreads], const uint16_t* __restrict__ base, long long stride,
                                         int row0, int limit)
{
    constexpr int CH = D / 8;
#pragma unroll
    for (int e = 0; e < ROWS * CH / kJtThreads; ++e) {
        const int c = threadIdx.x + e * kJtThreads;
        const int r = c / CH, ch = c - r * CH, row = row0 + r;
        stage[e] = make_uint4(0, 0, 0, 0);
        if (row < limit) stage[e] = *reinterpret_cast<const uint4*>(base + (long long)row * stride + ch * 8);
    }
}

// ... into LDS, D / 8 + 1 chunks to a row (one of padding).
template <int D, int ROWS>
__device__ __forceinline__ void jt_commit(uint4* __restrict__ lds, const uint4 (&stage)[ROWS * (D / 8) / kJtThreads])
{
    constexpr int CH = D / 8;
#pragma unroll
    for (int e = 0; e < ROWS * CH / kJtThreads; ++e) {
        const int c = threadIdx.x + e * kJtThreads;
        const int r = c / CH, ch = c - r * CH;
        lds[r * (CH + 1) + ch] = stage[e];
    }
}

template <int DT, int D>
__global__ __launch_bounds__(kJtThreads) void joint_stats_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_txt,
                                                                 const uint16_t* __restrict__ k_img, float2* __restrict__ stats, JtGeom g,
                                                                 float c)
{
    constexpr int CH = D / 8, KK = D / 16;
    __shared__ uint4 lds_k[2][kJtKeyTile * (CH + 1)];
    const int blocks = g.p_pad / kJtRows;
    const int s = blockIdx.x / blocks, i0 = (blockIdx.x - s * blocks) * kJtRows;
    const int b = s / g.heads, hd = s - b * g.heads;
    const uint16_t* qs = q + b * g.q_sb + hd * g.q_sh;
    const uint16_t* kts = k_txt + b * g.kt_sb + hd * g.kt_sh;
    const uint16_t* kis = k_img + b * g.ki_sb + hd * g.ki_sh;       // never dereferenced with Pk == 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;

    // the wave's 32 queries as the B operand: lane (r, half) holds Q[row r][16 kk + 8 half ..], kept for the whole walk
    const int qrow = i0 + wave * 32 + r;
    uint4 qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        qf[kk] = make_uint4(0, 0, 0, 0);
        if (qrow < g.P) qf[kk] = *reinterpret_cast<const uint4*>(qs + (long long)qrow * g.q_sp + kk * 16 + half * 8);
    }

    // the walk: tiles 0 .. n_txt - 1 are text keys, the rest image keys
    const int n_txt = (g.T + kJtKeyTile - 1) / kJtKeyTile, n_all = n_txt + (g.Pk + kJtKeyTile - 1) / kJtKeyTile;
    uint4 stage[kJtKeyTile * CH / kJtThreads];
    jt_fetch<D, kJtKeyTile>(stage, kts, g.kt_sp, 0, g.T);
    jt_commit<D, kJtKeyTile>(lds_k[0], stage);
    __syncthreads();

    float m = -INFINITY, negm = 0.f, l = 0.f;       // of this lane's half of the keys
    for (int t = 0; t < n_all; ++t) {
        const bool txt = t < n_txt;
        const int j0 = (txt ? t : t - n_txt) * kJtKeyTile, limit = txt ? g.T : g.Pk;
        if (t + 1 < n_all) {                        // the next tile's loads are in flight under this tile's MFMAs
            const bool ntxt = t + 1 < n_txt;
            jt_fetch<D, kJtKeyTile>(stage, ntxt ? kts : kis, ntxt ? g.kt_sp : g.ki_sp, (ntxt ? t + 1 : t + 1 - n_txt) * kJtKeyTile,
                                    ntxt ? g.T : g.Pk);
        }
        const uint4* cur = lds_k[t & 1];
#pragma unroll
        for (int sub = 0; sub < kJtKeyTile / 32; ++sub) {
            const int k0 = j0 + sub * 32;
            if (k0 >= limit) break;                 // no key at all in this step
            floatx16 x = {0};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) x = Mma32<DT>::run(cur[(sub * 32 + r) * (CH + 1) + kk * 2 + half], qf[kk], x);
            if (k0 + 32 > limit) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (k0 + acc_row(reg, half) >= limit) x[reg] = -INFINITY;
            }
            float top = x[0];
#pragma unroll
            for (int reg = 1; reg < 16; ++reg) top = fmaxf(top, x[reg]);
            const float m_new = fmaxf(m, top);
            const bool any = m_new > -INFINITY;
            const float negm_new = any ? -(m_new * c) : 0.f;
            const float carry = m > -INFINITY ? __builtin_amdgcn_exp2f(negm_new - negm) : 0.f;
            float part = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) part += __builtin_amdgcn_exp2f(__fmaf_rn(x[reg], c, negm_new));
            l = l * carry + part;
            m = m_new;
            negm = negm_new;
        }
        // buffer (t + 1) & 1 was last read in step t - 1, which every wave left through the barrier below
        if (t + 1 < n_all) jt_commit<D, kJtKeyTile>(lds_k[(t + 1) & 1], stage);
        __syncthreads();
    }
    // the two halves of the keys: the lower half's term first on both lanes
    const float m_o = __shfl_xor(m, 32), negm_o = __shfl_xor(negm, 32), l_o = __shfl_xor(l, 32);
    const float m_lo = half ? m_o : m, negm_lo = half ? negm_o : negm, l_lo = half ? l_o : l;
    const float m_hi = half ? m : m_o, negm_hi = half ? negm : negm_o, l_hi = half ? l : l_o;
    const float m_all = fmaxf(m_lo, m_hi);          // the lower half always holds text key 0: finite
    const float negm_all = -(m_all * c);
    const float t_lo = m_lo > -INFINITY ? l_lo * __builtin_amdgcn_exp2f(negm_all - negm_lo) : 0.f;
    const float t_hi = m_hi > -INFINITY ? l_hi * __builtin_amdgcn_exp2f(negm_all - negm_hi) : 0.f;
    if (half == 0) stats[(size_t)s * g.p_pad + qrow] = make_float2(negm_all, 1.0f / (t_lo + t_hi));
}

template <int DT, int D>
__global__ __launch_bounds__(kJtThreads) void joint_text_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_txt,
                                                                const float2* __restrict__ stats, float* __restrict__ sums, JtGeom g,
                                                                float c, float weight, int accumulate)
{
    constexpr int CH = D / 8, KK = D / 16;
    __shared__ uint4 lds_q[kJtRows * (CH + 1)];
    __shared__ uint4 lds_k[kJtKeyTile * (CH + 1)];
    const int cell_tiles = g.p_pad / kJtRows, txt_tiles = (g.T + kJtKeyTile - 1) / kJtKeyTile;
    const int plane = blockIdx.x / (cell_tiles * txt_tiles), rest = blockIdx.x - plane * (cell_tiles * txt_tiles);
    const int tt = rest / cell_tiles, ti = rest - tt * cell_tiles;
    const int t0 = tt * kJtKeyTile, i0 = ti * kJtRows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
    const int cell = i0 + wave * 32 + r;            // this lane's column; < p_pad

    floatx16 acc[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[mi] = floatx16{0};

    // the slices of this plane, ascending: every slice (plane 0 of one), or those of head `plane`
    for (int s = plane; s < g.n_slices; s += g.plane_step) {
        const int b = s / g.heads, hd = s - b * g.heads;
        uint4 stage_q[kJtRows * CH / kJtThreads], stage_k[kJtKeyTile * CH / kJtThreads];
        jt_fetch<D, kJtRows>(stage_q, q + b * g.q_sb + hd * g.q_sh, g.q_sp, i0, g.P);
        jt_fetch<D, kJtKeyTile>(stage_k, k_txt + b * g.kt_sb + hd * g.kt_sh, g.kt_sp, t0, g.T);
        const float2 st = stats[(size_t)s * g.p_pad + cell];
        __syncthreads();                            // the previous slice's reads are done
        jt_commit<D, kJtRows>(lds_q, stage_q);
        jt_commit<D, kJtKeyTile>(lds_k, stage_k);
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

template <int DT, int D>
void launch(hipStream_t s, const void* q, const void* k_txt, const void* k_img, float2* stats, float* sums, const JtGeom& g, int planes,
            float c, float weight, int accumulate)
{
    const unsigned blocks = (unsigned)(g.p_pad / kJtRows), txt_tiles = (unsigned)((g.T + kJtKeyTile - 1) / kJtKeyTile);
    hipLaunchKernelGGL((joint_stats_kernel<DT, D>), dim3(blocks * (unsigned)g.n_slices), dim3(kJtThreads), 0, s,
                       static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k_txt), static_cast<const uint16_t*>(k_img), stats, g, c);
    hipLaunchKernelGGL((joint_text_kernel<DT, D>), dim3(blocks * txt_tiles * (unsigned)planes), dim3(kJtThreads), 0, s,
                       static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k_txt), stats, sums, g, c, weight, accumulate);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_joint_tap_abi_version(void) { return DAAM_JOINT_TAP_ABI_VERSION; }

const char* daam_joint_tap_last_error(void) { return last_error; }

size_t daam_joint_tap_workspace(int batch, int heads, int P) { return stats_workspace(batch, heads, P); }

int daam_joint_tap_accumulate(const void* q, const void* k_txt, const void* k_img, int in_dtype, int batch, int heads, int P, int T, int Pk,
                              int d, int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_p, int64_t kt_stride_b, int64_t kt_stride_h,
                              int64_t kt_stride_t, int64_t ki_stride_b, int64_t ki_stride_h, int64_t ki_stride_p, float scale, float weight,
                              int accumulate, float* sums, int64_t sums_stride_h, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "joint_tap_accumulate";
    if (const int rc = check_shape(who, in_dtype, batch, heads, P)) return rc;
    if (T < 1 || T > kJtMaxT) return fail(DAAM_E_INVALID, "%s: T %d: 1..%d", who, T, kJtMaxT);
    if (Pk < 0 || Pk > kRowMaxP) return fail(DAAM_E_INVALID, "%s: Pk %d: 0..%d", who, Pk, kRowMaxP);
    if (d != 64 && d != 128) return fail(DAAM_E_INVALID, "%s: head dim %d: 64 or 128", who, d);
    if (const int rc = check_scale_weight(who, scale, weight)) return rc;
    if (!q || !k_txt || (Pk > 0 && !k_img) || !sums || !workspace)
        return fail(DAAM_E_INVALID, "%s: q, k_txt, k_img (with Pk > 0), sums and workspace must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_txt) | (Pk > 0 ? reinterpret_cast<uintptr_t>(k_img) : 0)) & 15)
        return fail(DAAM_E_INVALID, "%s: q, k_txt and k_img must be 16-byte aligned", who);
    if (const int rc = check_outputs_and_strides(who, sums, workspace, {q_stride_b, q_stride_h, q_stride_p, kt_stride_b, kt_stride_h, kt_stride_t,
                                                                       ki_stride_b, ki_stride_h, ki_stride_p}))
        return rc;
    if (q_stride_p < d || kt_stride_t < d || (Pk > 0 && ki_stride_p < d))
        return fail(DAAM_E_INVALID, "%s: row strides %lld / %lld / %lld below the head dim %d", who, (long long)q_stride_p,
                    (long long)kt_stride_t, (long long)ki_stride_p, d);
    const int64_t plane = (int64_t)T * P;
    if (sums_stride_h != 0 && sums_stride_h < plane)
        return fail(DAAM_E_INVALID, "%s: sums_stride_h %lld: 0 (one plane) or >= T * P = %lld", who, (long long)sums_stride_h, (long long)plane);
    if (sums_stride_h > ((int64_t)1 << 40)) return fail(DAAM_E_INVALID, "%s: sums_stride_h %lld is out of range", who, (long long)sums_stride_h);
    const int planes = sums_stride_h ? heads : 1;
    const size_t sums_bytes = sizeof(float) * ((size_t)(planes - 1) * (size_t)sums_stride_h + (size_t)plane);
    if (const int rc = check_workspace(who, batch, heads, P, sums, sums_bytes, workspace, workspace_bytes)) return rc;

    JtGeom g;
    g.heads = heads; g.P = P; g.T = T; g.Pk = Pk; g.n_slices = batch * heads; g.p_pad = pad_rows(P);
    g.plane_step = sums_stride_h ? heads : 1; g.plane_stride = sums_stride_h;
    g.q_sb = q_stride_b; g.q_sh = q_stride_h; g.q_sp = q_stride_p;
    g.kt_sb = kt_stride_b; g.kt_sh = kt_stride_h; g.kt_sp = kt_stride_t;
    g.ki_sb = Pk ? ki_stride_b : 0; g.ki_sh = Pk ? ki_stride_h : 0; g.ki_sp = Pk ? ki_stride_p : 0;
    const float c = log2e_scale(scale);
    const hipStream_t s = (hipStream_t)stream;
    float2* const stats = static_cast<float2*>(workspace);
    const void* const ki = Pk ? k_img : k_txt;                         // never read with Pk == 0
    const int acc = accumulate != 0;
    if (in_dtype == DAAM_F16) {
        if (d == 64) launch<DAAM_F16, 64>(s, q, k_txt, ki, stats, sums, g, planes, c, weight, acc);
        else launch<DAAM_F16, 128>(s, q, k_txt, ki, stats, sums, g, planes, c, weight, acc);
    } else {
        if (d == 64) launch<DAAM_BF16, 64>(s, q, k_txt, ki, stats, sums, g, planes, c, weight, acc);
        else launch<DAAM_BF16, 128>(s, q, k_txt, ki, stats, sums, g, planes, c, weight, acc);
    }
    return launched(who);
}
