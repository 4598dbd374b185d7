// daam_self_affinity_accumulate / daam_self_affinity_propagate (include/daam_self_affinity.h): the head-summed self-attention matrix of
// one attn1 call, added into a P x P f32 matrix, and the propagation of soft maps along that matrix.
//   * selfaff_stats_kernel<DT, DP>  : a workgroup of four waves owns 128 query rows of one slice, 32 per wave, and walks all keys in
//                                     tiles of 64 that go through LDS.  It computes K Q^T with mfma_f32_32x32x16 (keys on the
//                                     accumulator's rows, the wave's queries on the lanes), so a row's maximum and sum are reductions
//                                     over a lane's registers plus one exchange between the two lane halves at the very end.  Online:
//                                     per lane the running maximum m of the raw dot products and l = sum exp2(fma(raw, c, -(m c))),
//                                     c = f32(scale log2 e); padded keys count as -inf.  It writes (-(m c), 1 / l) per row.
//   * selfaff_sums_kernel<DT, DP>   : a workgroup owns a 128 x 128 tile of sums, four waves of 64 x 64 (2 x 2 MFMA blocks, queries on
//                                     the rows, keys on the lanes so that stores run along a row of sums).  It loops over the slices
//                                     in ascending order, recomputes the tile's dot products from Q and K tiles in LDS and adds
//                                     exp2(fma(raw, c, -(m c))) * (1 / l) with one fma into 64 accumulators per lane that stay in
//                                     registers across the whole loop; one read-modify-write of sums at the end.
//   * selfaff_propagate_kernel<NMAX, ROWS, FIRST>, selfaff_copy_kernel: a wave owns ROWS rows of sums (2 with up to 16 maps,
//                                     else 1), each summed in the header's order; a map value is loaded once for the
//                                     wave's rows; the first iteration of a call forms the row sums in the same pass.
// d = 40 / 80 / 160 are the same templates with the depth zero-padded to a multiple of 16 in LDS (DP = 48 / 80 / 160); a depth above
// 80 goes through LDS in two halves.  Rows past P are zero-filled in LDS, masked in the statistics and not stored in the epilogue.
// No atomics, no dependence on the grid: two runs give the same bits.
#include "../../include/daam_self_affinity.h"
#include "daam_rowsoftmax32.h"

namespace daam {

constexpr int kSaMaxMaps = 32;
constexpr int kSaMaxIterations = 16;
constexpr int kSaThreads = 256;
constexpr int kSaTile = kRowTile;                   // rows of a statistics block, rows and columns of a tile of sums
constexpr int kSaKeyTile = 64;                      // keys per step of the statistics walk

struct SaGeom {
    int heads, P, d, n_slices;
    int p_pad;                                      // P rounded up to whole tiles: the row count of a slice's statistics
    long long q_sb, q_sh, q_sp, k_sb, k_sh, k_sp;
};

// ROWS rows x DC elements of depth, from depth `depth0` on, of a [P][d] matrix with row stride `stride` into LDS as 16-byte chunks,
// DC / 8 + 1 chunks to a row (one of padding).  Rows >= P and depth >= d are zero.
template <int DC, int ROWS>
__device__ __forceinline__ void sa_load_tile(uint4* __restrict__ lds, const uint16_t* __restrict__ base, long long stride, int row0,
                                             int depth0, int P, int d)
{
    constexpr int CH = DC / 8;
    for (int c = threadIdx.x; c < ROWS * CH; c += kSaThreads) {
        const int r = c / CH, ch = c - r * CH;
        const int row = row0 + r, depth = depth0 + ch * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < P && depth < d) v = *reinterpret_cast<const uint4*>(base + (long long)row * stride + depth);
        lds[r * (CH + 1) + ch] = v;
    }
}

template <int DT, int DP>
__global__ __launch_bounds__(kSaThreads) void selfaff_stats_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                                   float2* __restrict__ stats, SaGeom g, float c)
{
    constexpr int CH = DP / 8, KK = DP / 16;
    __shared__ uint4 lds_k[kSaKeyTile * (CH + 1)];
    const int blocks = g.p_pad / kSaTile;
    const int s = blockIdx.x / blocks, i0 = (blockIdx.x - s * blocks) * kSaTile;
    const int b = s / g.heads, hd = s - b * g.heads;
    const uint16_t* qs = q + b * g.q_sb + hd * g.q_sh;
    const uint16_t* ks = k + b * g.k_sb + hd * g.k_sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;

    // the wave's 32 queries as the B operand: lane (r, half) holds Q[row r][16 kk + 8 half ..], kept for the whole walk
    const int qrow = i0 + wave * 32 + r;
    uint4 qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        const int depth = kk * 16 + half * 8;
        qf[kk] = make_uint4(0, 0, 0, 0);
        if (qrow < g.P && depth < g.d) qf[kk] = *reinterpret_cast<const uint4*>(qs + (long long)qrow * g.q_sp + depth);
    }

    float m = -INFINITY, negm = 0.f, l = 0.f;       // of this lane's half of the keys
    for (int j0 = 0; j0 < g.P; j0 += kSaKeyTile) {
        __syncthreads();
        sa_load_tile<DP, kSaKeyTile>(lds_k, ks, g.k_sp, j0, 0, g.P, g.d);
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < kSaKeyTile / 32; ++sub) {
            floatx16 x = {0};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) x = Mma32<DT>::run(lds_k[(sub * 32 + r) * (CH + 1) + kk * 2 + half], qf[kk], x);
            float top = -INFINITY;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                if (j0 + sub * 32 + acc_row(reg, half) >= g.P) x[reg] = -INFINITY;
                top = fmaxf(top, x[reg]);
            }
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
    }
    // the two halves of the keys: the lower half's term first on both lanes
    const float m_o = __shfl_xor(m, 32), negm_o = __shfl_xor(negm, 32), l_o = __shfl_xor(l, 32);
    const float m_lo = half ? m_o : m, negm_lo = half ? negm_o : negm, l_lo = half ? l_o : l;
    const float m_hi = half ? m : m_o, negm_hi = half ? negm : negm_o, l_hi = half ? l : l_o;
    const float m_all = fmaxf(m_lo, m_hi);          // the lower half always holds key 0: finite
    const float negm_all = -(m_all * c);
    const float t_lo = m_lo > -INFINITY ? l_lo * __builtin_amdgcn_exp2f(negm_all - negm_lo) : 0.f;
    const float t_hi = m_hi > -INFINITY ? l_hi * __builtin_amdgcn_exp2f(negm_all - negm_hi) : 0.f;
    if (half == 0) stats[(size_t)s * g.p_pad + qrow] = make_float2(negm_all, 1.0f / (t_lo + t_hi));
}

template <int DT, int DP>
__global__ __launch_bounds__(kSaThreads) void selfaff_sums_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                                  const float2* __restrict__ stats, float* __restrict__ sums, SaGeom g,
                                                                  float c, float weight, int accumulate)
{
    constexpr int DC = DP > 80 ? DP / 2 : DP;       // depth per pass through LDS
    constexpr int CH = DC / 8, KK = DC / 16;
    static_assert(DC % 16 == 0, "a depth pass is whole MFMA steps");
    __shared__ uint4 lds_q[kSaTile * (CH + 1)];
    __shared__ uint4 lds_k[kSaTile * (CH + 1)];
    __shared__ float2 lds_stat[kSaTile];
    const int tiles = g.p_pad / kSaTile;
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    const int i0 = ti * kSaTile, j0 = tj * kSaTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    floatx16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = floatx16{0};

    for (int s = 0; s < g.n_slices; ++s) {
        const int b = s / g.heads, hd = s - b * g.heads;
        const uint16_t* qs = q + b * g.q_sb + hd * g.q_sh;
        const uint16_t* ks = k + b * g.k_sb + hd * g.k_sh;
        floatx16 x[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) x[mi][ni] = floatx16{0};
#pragma unroll
        for (int depth0 = 0; depth0 < DP; depth0 += DC) {
            __syncthreads();
            sa_load_tile<DC, kSaTile>(lds_q, qs, g.q_sp, i0, depth0, g.P, g.d);
            sa_load_tile<DC, kSaTile>(lds_k, ks, g.k_sp, j0, depth0, g.P, g.d);
            if (depth0 == 0 && threadIdx.x < kSaTile) lds_stat[threadIdx.x] = stats[(size_t)s * g.p_pad + i0 + threadIdx.x];
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                uint4 a[2], bf[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) a[mi] = lds_q[(wr * 64 + mi * 32 + r) * (CH + 1) + kk * 2 + half];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) bf[ni] = lds_k[(wc * 64 + ni * 32 + r) * (CH + 1) + kk * 2 + half];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) x[mi][ni] = Mma32<DT>::run(a[mi], bf[ni], x[mi][ni]);
            }
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float2 st = lds_stat[wr * 64 + mi * 32 + acc_row(reg, half)];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[mi][ni][reg] = add_prob(x[mi][ni][reg], c, st, acc[mi][ni][reg]);
            }
    }

#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = i0 + wr * 64 + mi * 32 + acc_row(reg, half);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int col = j0 + wc * 64 + ni * 32 + r;
                if (row < g.P && col < g.P) store_weighted(sums + (size_t)row * g.P + col, weight, acc[mi][ni][reg], accumulate);
            }
        }
}

// The sum over a wave of one value per lane, the same bits on every lane: a butterfly over the lane distances 32 .. 1.
__device__ __forceinline__ float sa_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

constexpr int kSaWaves = kSaThreads / 64;

// Rows of sums per wave: a map value is loaded once and feeds that many rows, while the accumulators (rows x NMAX) stay in registers.
// Two rows and two steps of the walk in flight are what measured best at P = 4096 with 8 maps (four rows leave a CU four waves, four
// steps cost more registers than they hide latency: DESIGN 3.22).
constexpr int sa_rows(int nmax) { return nmax <= 16 ? 2 : 1; }

// One wave owns ROWS consecutive rows of sums; a row's order of summation is the header's whatever ROWS is.  FIRST: the call's first
// iteration, which also forms the row sums (in the same pass over sums) and leaves them in the workspace for the iterations after it.
template <int NMAX, int ROWS, bool FIRST>
__global__ __launch_bounds__(kSaThreads) void selfaff_propagate_kernel(const float* __restrict__ sums, float* __restrict__ rowsum,
                                                                       const float* __restrict__ src, float* __restrict__ dst, int P,
                                                                       int n_maps)
{
    const int i0 = (blockIdx.x * kSaWaves + (threadIdx.x >> 6)) * ROWS, lane = threadIdx.x & 63;
    if (i0 >= P) return;
    const float* row[ROWS];                         // wave-uniform; spare slots re-read the last row and store nothing
#pragma unroll
    for (int r = 0; r < ROWS; ++r) row[r] = sums + (size_t)min(i0 + r, P - 1) * P;
    const float* maps[NMAX];                        // wave-uniform; spare slots re-read the last map
#pragma unroll
    for (int n = 0; n < NMAX; ++n) maps[n] = src + (size_t)min(n, n_maps - 1) * P;
    float acc[ROWS][NMAX], part[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        part[r] = 0.f;
#pragma unroll
        for (int n = 0; n < NMAX; ++n) acc[r][n] = 0.f;
    }
#pragma unroll 2
    for (int j = lane; j < P; j += 64) {
        float a[ROWS], mv[NMAX];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) a[r] = row[r][j];
#pragma unroll
        for (int n = 0; n < NMAX; ++n) mv[n] = maps[n][j];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (FIRST) part[r] += a[r];
#pragma unroll
            for (int n = 0; n < NMAX; ++n) acc[r][n] = __fmaf_rn(a[r], mv[n], acc[r][n]);
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int i = i0 + r;
        if (i >= P) break;
        float total;
        if (FIRST) {
            total = sa_wave_sum(part[r]);
            if (lane == 63) rowsum[i] = total;
        } else {
            total = rowsum[i];
        }
#pragma unroll
        for (int n = 0; n < NMAX; ++n) {
            const float v = sa_wave_sum(acc[r][n]);
            if (n < n_maps && lane == (n & 63)) dst[(size_t)n * P + i] = total == 0.f ? maps[n][i] : v / total;
        }
    }
}

__global__ __launch_bounds__(kSaThreads) void selfaff_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int count)
{
    const int p = blockIdx.x * kSaThreads + threadIdx.x;
    if (p < count) dst[p] = src[p];
}

namespace {

template <int DT, int DP>
void launch_accumulate(hipStream_t s, const void* q, const void* k, float2* stats, float* sums, const SaGeom& g, float c, float weight,
                       int accumulate)
{
    const unsigned blocks = (unsigned)(g.p_pad / kSaTile);
    hipLaunchKernelGGL((selfaff_stats_kernel<DT, DP>), dim3(blocks * (unsigned)g.n_slices), dim3(kSaThreads), 0, s,
                       static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k), stats, g, c);
    hipLaunchKernelGGL((selfaff_sums_kernel<DT, DP>), dim3(blocks * blocks), dim3(kSaThreads), 0, s, static_cast<const uint16_t*>(q),
                       static_cast<const uint16_t*>(k), stats, sums, g, c, weight, accumulate);
}

template <int DT>
void launch_accumulate_depth(hipStream_t s, const void* q, const void* k, float2* stats, float* sums, const SaGeom& g, float c,
                             float weight, int accumulate)
{
    if (g.d == 40) launch_accumulate<DT, 48>(s, q, k, stats, sums, g, c, weight, accumulate);
    else if (g.d == 64) launch_accumulate<DT, 64>(s, q, k, stats, sums, g, c, weight, accumulate);
    else if (g.d == 80) launch_accumulate<DT, 80>(s, q, k, stats, sums, g, c, weight, accumulate);
    else launch_accumulate<DT, 160>(s, q, k, stats, sums, g, c, weight, accumulate);
}

template <int NMAX>
void launch_propagate(hipStream_t s, const float* sums, float* rowsum, const float* src, float* dst, int P, int n_maps, bool first)
{
    constexpr int ROWS = sa_rows(NMAX), per_block = kSaWaves * ROWS;
    const dim3 grid((unsigned)((P + per_block - 1) / per_block)), block(kSaThreads);
    if (first) hipLaunchKernelGGL((selfaff_propagate_kernel<NMAX, ROWS, true>), grid, block, 0, s, sums, rowsum, src, dst, P, n_maps);
    else hipLaunchKernelGGL((selfaff_propagate_kernel<NMAX, ROWS, false>), grid, block, 0, s, sums, rowsum, src, dst, P, n_maps);
}

}  // namespace

}  // namespace daam

using namespace daam;

int daam_self_affinity_abi_version(void) { return DAAM_SELF_AFFINITY_ABI_VERSION; }

const char* daam_self_affinity_last_error(void) { return last_error; }

size_t daam_self_affinity_workspace(int batch, int heads, int P) { return stats_workspace(batch, heads, P); }

size_t daam_self_affinity_propagate_workspace(int N, int P)
{
    if (N < 1 || N > kSaMaxMaps || P < 1 || P > kRowMaxP) return 0;
    return round8(sizeof(float) * ((size_t)N + 1) * P);
}

int daam_self_affinity_accumulate(const void* q, const void* k, int in_dtype, int batch, int heads, int P, int d, int64_t q_stride_b,
                                  int64_t q_stride_h, int64_t q_stride_p, int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_p,
                                  float scale, float weight, int accumulate, float* sums, void* workspace, size_t workspace_bytes,
                                  void* stream)
{
    const char* who = "self_affinity_accumulate";
    if (const int rc = check_shape(who, in_dtype, batch, heads, P)) return rc;
    if (d != 40 && d != 64 && d != 80 && d != 160) return fail(DAAM_E_INVALID, "%s: head dim %d: 40, 64, 80 or 160", who, d);
    if (const int rc = check_scale_weight(who, scale, weight)) return rc;
    if (!q || !k || !sums || !workspace) return fail(DAAM_E_INVALID, "%s: q, k, sums and workspace must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15)
        return fail(DAAM_E_INVALID, "%s: q and k must be 16-byte aligned", who);
    if (const int rc = check_outputs_and_strides(who, sums, workspace, {q_stride_b, q_stride_h, q_stride_p, k_stride_b, k_stride_h, k_stride_p}))
        return rc;
    if (q_stride_p < d || k_stride_p < d)
        return fail(DAAM_E_INVALID, "%s: row strides %lld / %lld below the head dim %d", who, (long long)q_stride_p, (long long)k_stride_p, d);
    if (const int rc = check_workspace(who, batch, heads, P, sums, sizeof(float) * (size_t)P * P, workspace, workspace_bytes)) return rc;

    SaGeom g;
    g.heads = heads; g.P = P; g.d = d; g.n_slices = batch * heads; g.p_pad = pad_rows(P);
    g.q_sb = q_stride_b; g.q_sh = q_stride_h; g.q_sp = q_stride_p;
    g.k_sb = k_stride_b; g.k_sh = k_stride_h; g.k_sp = k_stride_p;
    const float c = log2e_scale(scale);
    const hipStream_t s = (hipStream_t)stream;
    float2* const stats = static_cast<float2*>(workspace);
    if (in_dtype == DAAM_F16) launch_accumulate_depth<DAAM_F16>(s, q, k, stats, sums, g, c, weight, accumulate != 0);
    else launch_accumulate_depth<DAAM_BF16>(s, q, k, stats, sums, g, c, weight, accumulate != 0);
    return launched(who);
}

int daam_self_affinity_propagate(const float* sums, int P, const float* maps, int N, int iterations, float* refined, void* workspace,
                                 size_t workspace_bytes, void* stream)
{
    const char* who = "self_affinity_propagate";
    if (P < 1 || P > kRowMaxP) return fail(DAAM_E_INVALID, "%s: P %d: 1..%d", who, P, kRowMaxP);
    if (N < 1 || N > kSaMaxMaps) return fail(DAAM_E_INVALID, "%s: %d maps: 1..%d", who, N, kSaMaxMaps);
    if (iterations < 0 || iterations > kSaMaxIterations)
        return fail(DAAM_E_INVALID, "%s: %d iterations: 0..%d", who, iterations, kSaMaxIterations);
    if (!sums || !maps || !refined || !workspace)
        return fail(DAAM_E_INVALID, "%s: sums, maps, refined and workspace must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(refined) |
         reinterpret_cast<uintptr_t>(workspace)) & 3)
        return fail(DAAM_E_INVALID, "%s: sums, maps, refined and workspace must be 4-byte aligned", who);
    const size_t need = daam_self_affinity_propagate_workspace(N, P);
    if (workspace_bytes < need)
        return fail(DAAM_E_INVALID, "%s: workspace of %zu bytes: %d maps of %d cells need %zu", who, workspace_bytes, N, P, need);
    const size_t bytes = sizeof(float) * (size_t)N * P;
    if (overlap(refined, bytes, maps, bytes)) return fail(DAAM_E_INVALID, "%s: refined overlaps maps", who);
    if (overlap(refined, bytes, workspace, workspace_bytes)) return fail(DAAM_E_INVALID, "%s: refined overlaps the workspace", who);
    // the launches read maps and sums while they write refined and the workspace
    if (overlap(maps, bytes, workspace, workspace_bytes)) return fail(DAAM_E_INVALID, "%s: maps overlap the workspace", who);
    const size_t sums_bytes = sizeof(float) * (size_t)P * P;
    if (overlap(sums, sums_bytes, refined, bytes)) return fail(DAAM_E_INVALID, "%s: sums overlap refined", who);
    if (overlap(sums, sums_bytes, workspace, workspace_bytes)) return fail(DAAM_E_INVALID, "%s: sums overlap the workspace", who);

    const hipStream_t s = (hipStream_t)stream;
    if (iterations == 0) {
        hipLaunchKernelGGL(selfaff_copy_kernel, dim3((unsigned)((N * P + kSaThreads - 1) / kSaThreads)), dim3(kSaThreads), 0, s, maps, refined,
                           N * P);
    } else {
        float* const scratch = static_cast<float*>(workspace);
        float* const rowsum = scratch + (size_t)N * P;
        const float* src = maps;
        for (int t = 0; t < iterations; ++t) {
            // the last launch writes refined, the one before it the scratch, and so on back to the first
            float* const dst = (iterations - 1 - t) % 2 == 0 ? refined : scratch;
            if (N <= 1) launch_propagate<1>(s, sums, rowsum, src, dst, P, N, t == 0);
            else if (N <= 2) launch_propagate<2>(s, sums, rowsum, src, dst, P, N, t == 0);
            else if (N <= 4) launch_propagate<4>(s, sums, rowsum, src, dst, P, N, t == 0);
            else if (N <= 8) launch_propagate<8>(s, sums, rowsum, src, dst, P, N, t == 0);
            else if (N <= 16) launch_propagate<16>(s, sums, rowsum, src, dst, P, N, t == 0);
            else launch_propagate<32>(s, sums, rowsum, src, dst, P, N, t == 0);
            src = dst;
        }
    }
    return launched(who);
}
