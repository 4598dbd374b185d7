// Paired head_dim-64 tap (probes): one workgroup runs TWO chains over the same recorded Q -- the generation's chain or a
// probe's (chain A: its per-step K, double-buffered by LDS-DMA as in tap_d64_kernel) and a probe's (chain B: one fixed K tile,
// DMA'd into LDS once at workgroup start).  Each step's Q tile is fetched from HBM once and feeds both MFMA chains; the
// softmax and the accumulate run per chain, into two register sets of running sums.  Chain B re-reads the step's Q operands from the
// wave's LDS tile after chain A's softmax (the Q of the next step is requested only then), which keeps the kernel at 128 VGPRs with no
// scratch: two eight-wave workgroups per CU, four waves per SIMD, like tap_d64_kernel.
//
// Every sum set is bit-identical to running its chain alone through tap_d64_kernel<InF16, ACC_T, FAST, true, 8>: the same tiling (eight
// waves, 256 pixels of one kept head) and the same tile (daam_tap_tile64.h: geometry, swizzle, descriptor, prologue, the MFMA chain per
// chain).  This file adds the second chain, its fixed K tile and the second set of sums.
// LDS: 2 K buffers (20 KiB) + 8 Q tiles (32 KiB) + the fixed K tile (10 KiB) + step pointers (1 KiB) = 63 KiB: two workgroups per CU.
#include "daam_tap16_softmax.h"
#include "daam_tap_tile64.h"

namespace daam {
namespace tap_pair {

constexpr int kWaves = 8;
constexpr int kFixOff = kTapQOff + kWaves * kTapQTile;   // behind the tile's K buffers and Q tiles: chain B's fixed K tile

template <typename ACC_T> constexpr size_t lds_bytes() {
    const size_t kb = (size_t)kFixOff + kTapKBuf, st = (size_t)kTok * (32 * kWaves) * sizeof(ACC_T);
    return (kb > st ? kb : st) + (size_t)kMaxStepsPerLaunch * 2 * sizeof(void*);
}

}  // namespace tap_pair

// L.layers = [n_layers chain-A entries (wg_begin ascending)][n_layers chain-B entries, same order]; L.ptrs: chain A's (q, k) per step, and
// chain B's entry ptr_begin points at ONE pointer pair whose k is its fixed key (its q is chain A's, step by step, checked by the host).
// Both chains of an entry share hw, heads, head_dim 64, q strides, k_sh / k_st, scale and round_logits (the host pairs only such chains).
template <typename ACC_T, bool FAST_EXP>
__global__ __launch_bounds__(512, 4) void tap_pair_kernel(const TapLaunch L)
{
    using namespace tap_pair;
    using IN = InF16;
    constexpr int NT = 64 * kWaves;
    constexpr int TILE = 32 * kWaves;
    constexpr int VEC = AccVec<ACC_T>::kPerVec;
    constexpr int PPR = TILE / VEC;
    constexpr size_t kPtrOff = lds_bytes<ACC_T>() - (size_t)kMaxStepsPerLaunch * 2 * sizeof(void*);

    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* kbuf = smem;
    unsigned char* kfix = smem + kFixOff;
    ACC_T* stage = reinterpret_cast<ACC_T*>(smem);            // [kTok][TILE], aliases the K / Q buffers (not the fixed tile's tail)
    const void** sptr = reinterpret_cast<const void**>(smem + kPtrOff);

    const int wg = mfma_logical_block(L.total_wgs, L.wgs_per_xcd);
    if (wg < 0) return;
    tap_mark_started(L);
    const DAAM_GLOBAL TapLayer* gl = as_global<TapLayer>(L.layers);
    const int li = mfma_find_layer(gl, L.n_layers, wg);
    TapLayer lay, layb;
    load_layer(gl + li, &lay);
    load_layer(gl + L.n_layers + li, &layb);
    const int tid = threadIdx.x;
    tap_step_ptrs_to_lds<NT>(L, lay, true, sptr, tid);
    const void* kb_ptr = as_global<TapPtr>(L.ptrs)[layb.ptr_begin].k;
    const int n_steps = lay.n_steps;
    // tap_tile_decode (daam_tap_tile64.h) plus chain B's K offset, kept as text: through the function both instances come out as other machine code
    const int rel = wg - lay.wg_begin;
    const int kh = rel / lay.tiles_per_head;
    const int p0 = (rel - kh * lay.tiles_per_head) * TILE;
    const int bh = lay.bh_first + kh;
    const int b = bh / lay.heads, hd = bh - b * lay.heads;
    const int64_t k_off = b * lay.k_sb + hd * lay.k_sh;
    const int64_t kb_off = b * layb.k_sb + hd * layb.k_sh;
    const int64_t q_off = b * lay.q_sb + hd * lay.q_sh;

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, h = lane >> 4;

    // ---- running sums of both chains -> registers (through the staging tile) -----------------------
    typename Pair<ACC_T>::T run0[kSlots16 / 2], run1[kSlots16 / 2], rb0[kSlots16 / 2], rb1[kSlots16 / 2];
    ACC_T* acc = reinterpret_cast<ACC_T*>(lay.acc) + (size_t)kh * kTok * lay.hw;
    ACC_T* accb = reinterpret_cast<ACC_T*>(layb.acc) + (size_t)kh * kTok * lay.hw;
    auto read_in = [&](const ACC_T* src, bool fresh, typename Pair<ACC_T>::T (&r0)[kSlots16 / 2], typename Pair<ACC_T>::T (&r1)[kSlots16 / 2]) {
        if (!fresh) {
            for (int piece = tid; piece < kTok * PPR; piece += NT) {
                const int row = piece / PPR, col = (piece - row * PPR) * VEC;
                if (p0 + col < lay.hw)
                    *reinterpret_cast<float4v*>(stage + row * TILE + col) = *as_global<float4v>(src + (size_t)row * lay.hw + p0 + col);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kSlots16; ++i) {
                const int t = slot16_token(i, h);
                r0[i >> 1][i & 1] = t < kTok ? from_acc<ACC_T>(stage[t * TILE + wave * 32 + j]) : 0;
                r1[i >> 1][i & 1] = t < kTok ? from_acc<ACC_T>(stage[t * TILE + wave * 32 + 16 + j]) : 0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kSlots16; ++i) { r0[i >> 1][i & 1] = 0; r1[i >> 1][i & 1] = 0; }
        }
        __syncthreads();
    };
    read_in(acc, lay.fresh != 0, run0, run1);
    read_in(accb, layb.fresh != 0, rb0, rb1);
    // K rows 77..79 of the two step buffers are never written by a step: zero them once (the DMAs below re-read row 76 into them for
    // the fixed tile, exactly as for a step buffer)
    tap64_zero_pad_rows<NT>(kbuf, tid);

    const unsigned k_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(k_off * 2));
    const unsigned kb_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(kb_off * 2));
    const int q_rows_in = __builtin_amdgcn_readfirstlane(lay.hw - (p0 + wave * 32));
    const unsigned q_step8 = (unsigned)__builtin_amdgcn_readfirstlane(8 * (int)lay.q_sp * 2);
    unsigned q_s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q_s[i] = 8 * i < q_rows_in ? (unsigned)i * q_step8 : 0u;
    unsigned char* qtile = kbuf + kTapQOff + wave * kTapQTile;
    const int f_rd = j * kTapRow + swz_chunk(j, h);
    unsigned kd_src[3];
#pragma unroll
    for (int j2 = 0; j2 < 3; ++j2) {
        const int blk = kWaves * j2 + wave;
        const int row = min(8 * blk + (lane >> 3), kTok - 1);
        const int ch = (lane & 7) ^ (((8 * blk + (lane >> 3)) >> 1) & 7);
        kd_src[j2] = (unsigned)((row * (int)lay.k_st + ch * 8) * 2);
    }
    unsigned qd_src[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int ch = (lane & 7) ^ ((4 * par + (lane >> 4)) & 7);
        const int px = p0 + wave * 32 + (lane >> 3);
        qd_src[par] = (unsigned)((q_off + (int64_t)min(px, lay.hw - 1) * lay.q_sp) * 2) + (unsigned)ch * 16u;
    }
    const floatx4 cmask = premask_tile4(h);
    auto step = [&](int s) {
        __syncthreads();
        const unsigned char* kb = kbuf + (s & 1) * kTapKBuf;
        const int s_fetch = min(s + 1, n_steps - 1);
        tap64_dma_k<kWaves>(sptr[2 * s_fetch + 1], k_base, kbuf + ((s + 1) & 1) * kTapKBuf, wave, kd_src);
        floatx4 c0[5], c1[5];
        {
            const half8 q00 = *reinterpret_cast<const half8*>(qtile + f_rd), q01 = *reinterpret_cast<const half8*>(qtile + (f_rd ^ 64));
            const half8 q10 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + f_rd);
            const half8 q11 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + (f_rd ^ 64));
            tap64_mfma_chain<IN>(kb, f_rd, q00, q01, q10, q11, cmask, c0, c1);
        }
        softmax20_accumulate<ACC_T, FAST_EXP, true>(c0, lay, h, run0);
        softmax20_accumulate<ACC_T, FAST_EXP, true>(c1, lay, h, run1);
        // chain B reads the same Q operands again from the wave's tile (16 VGPRs fewer than holding them across chain A's softmax: no
        // spills at 128 VGPRs); only then may the next step's Q land there
        asm volatile("" ::: "memory");
        {
            const half8 q00 = *reinterpret_cast<const half8*>(qtile + f_rd), q01 = *reinterpret_cast<const half8*>(qtile + (f_rd ^ 64));
            const half8 q10 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + f_rd);
            const half8 q11 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + (f_rd ^ 64));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            tap64_dma_q(sptr[2 * s_fetch], qtile, qd_src, q_s);
            tap64_mfma_chain<IN>(kfix, f_rd, q00, q01, q10, q11, cmask, c0, c1);
        }
        softmax20_accumulate<ACC_T, FAST_EXP, true>(c0, layb, h, rb0);
        softmax20_accumulate<ACC_T, FAST_EXP, true>(c1, layb, h, rb1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    tap64_dma_k<kWaves>(sptr[1], k_base, kbuf, wave, kd_src);
    tap64_dma_k<kWaves>(kb_ptr, kb_base, kfix, wave, kd_src);
    tap64_dma_q(sptr[0], qtile, qd_src, q_s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int s = 0; s < n_steps; ++s) step(s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- write back both chains: registers -> LDS [token][pixel] -> 16-byte row pieces ----------------
    auto write_out = [&](ACC_T* dst, const typename Pair<ACC_T>::T (&r0)[kSlots16 / 2], const typename Pair<ACC_T>::T (&r1)[kSlots16 / 2]) {
#pragma unroll
        for (int i = 0; i < kSlots16; ++i) {
            const int t = slot16_token(i, h);
            if (t < kTok) {
                stage[t * TILE + wave * 32 + j] = to_acc<ACC_T>(r0[i >> 1][i & 1]);
                stage[t * TILE + wave * 32 + 16 + j] = to_acc<ACC_T>(r1[i >> 1][i & 1]);
            }
        }
        __syncthreads();
        for (int piece = tid; piece < kTok * PPR; piece += NT) {
            const int row = piece / PPR, col = (piece - row * PPR) * VEC;
            if (p0 + col < lay.hw)
                *as_global_rw<float4v>(dst + (size_t)row * lay.hw + p0 + col) = *reinterpret_cast<const float4v*>(stage + row * TILE + col);
        }
        __syncthreads();
    };
    write_out(acc, run0, run1);
    write_out(accb, rb0, rb1);
}

int tap_pair_tile_pixels() { return 32 * tap_pair::kWaves; }

hipError_t launch_tap_pair(const TapLaunch& L, int fast_exp, hipStream_t stream, int* grid_out, int* lds_out)
{
    const int grid = L.wgs_per_xcd * 8;
    *grid_out = grid;
    const size_t lds = tap_pair::lds_bytes<_Float16>();
    *lds_out = (int)lds;
    const void* fn = fast_exp ? reinterpret_cast<const void*>(tap_pair_kernel<_Float16, true>)
                              : reinterpret_cast<const void*>(tap_pair_kernel<_Float16, false>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (fast_exp) hipLaunchKernelGGL((tap_pair_kernel<_Float16, true>), dim3(grid), dim3(512), lds, stream, L);
    else hipLaunchKernelGGL((tap_pair_kernel<_Float16, false>), dim3(grid), dim3(512), lds, stream, L);
    return hipGetLastError();
}

}  // namespace daam
