// The head_dim-64 tile of the tap kernels, once: 128-byte swizzled K / Q rows in LDS, their LDS-DMA fetch one step ahead, the 5 x 4 MFMA
// chain into 20 token slots per lane and the softmax dispatch.  Built from it:
//   tap_d64_kernel   (daam_tap_d64.hip)    the tile itself; adds the step protocols and the register-staged head_dim < 64 form
//   tap_walk_kernel  (daam_tap_walk.hip)   adds the window loop and a staging tile of its own
//   tap_pair_kernel  (daam_tap_pair.hip)   adds a second chain over a fixed K tile
//   tap_chunk_kernel (daam_tap_chunk.hip)  adds the walk over 64-element chunks of a longer head_dim
// tap_wide_kernel, tap_mfma_kernel and the slab kernel have tilings of their own and take the prologue or the descriptor from here.
// Everything is constexpr or __device__ __forceinline__.  A kernel calls a function of this file only where every instance of it stays
// byte for byte what it was with the text in place; profiles/tile64_refactor.json has the trial of every (piece, kernel) pair, with
// the size / register difference seen.  Still text in the kernels after those trials: the DMA source set-up (every kernel), the K DMA
// issue in d64 and walk (dma_q and pair's dma_k are calls), the staging-tile path of the running sums (every kernel), the operand-read offset,
// the workgroup decode in pair.  chunk and wide reach tap_tensor_rsrc through a one-line lambda: called directly it changes them.
#pragma once
#include "daam_tap16_softmax.h"

namespace daam {

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
constexpr int kTapRow = 128;                        // bytes per K / Q row in LDS (head_dim 64 x 2 bytes), chunks swizzled
constexpr int kTapKBuf = kD64Rows * kTapRow;        // 10240: 80 K rows, rows 77..79 stay finite
constexpr int kTapQTile = 32 * kTapRow;             // 4096: one wave's 32 pixel rows
constexpr int kTapQOff = 2 * kTapKBuf;              // the waves' Q tiles follow the two K buffers

// byte offset of 16-byte chunk `chunk` inside row `row` of a swizzled [rows][128 B] image: XOR with (row >> 1) & 7 makes the operand
// reads (16 rows x one chunk per ds_read_b128) conflict-free without padding
__device__ __forceinline__ constexpr int swz_chunk(int row, int chunk) { return ((chunk ^ ((row >> 1) & 7)) << 4); }

// the dtype pairs the eight-wave (256-pixel) form exists for: fp16 Q / K with fp16 or f32 sums, bf16 Q / K with bf16 or f32 sums
constexpr bool tap_tile64_has_waves8(int in_dtype, int acc_dtype)
{
    return (in_dtype == 0 && (acc_dtype == 0 || acc_dtype == 1)) || (in_dtype == 2 && (acc_dtype == 2 || acc_dtype == 1));
}

// ---- descriptor ----------------------------------------------------------------------------------------------------------------------
// Fetches are raw buffer loads: address = the step's tensor (a wave-uniform resource descriptor built from the pointer
// in SGPRs) + a per-lane 32-bit byte offset that never changes + a wave-uniform byte offset.  No 64-bit address
// arithmetic on the VALU (7 v_lshl_add_u64 per wave-step with plain global loads), offsets stay single registers.
typedef __attribute__((address_space(3))) void* lds_ptr_t;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tap_tensor_rsrc(const void* p)
{
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, -1, 0x00020000);
}

// ---- prologue ------------------------------------------------------------------------------------------------------------------------
// per-step q / k base pointers -> LDS once, so the step loop never waits on a dependent global load (table fetch -> address -> data)
// on its critical path.  `table`: the launch has a layer table (else its one step is L.one_ptr).  NT = threads per workgroup.
template <int NT>
__device__ __forceinline__ void tap_step_ptrs_to_lds(const TapLaunch& L, const TapLayer& lay, bool table, const void** sptr, int tid)
{
    if (table) {
        const DAAM_GLOBAL TapPtr* ptrs = as_global<TapPtr>(L.ptrs) + lay.ptr_begin;
        for (int i = tid; i < lay.n_steps; i += NT) {
            sptr[2 * i] = ptrs[i].q;
            sptr[2 * i + 1] = ptrs[i].k;
        }
    } else if (tid == 0) {
        sptr[0] = L.one_ptr.q;
        sptr[1] = L.one_ptr.k;
    }
}

// workgroup -> kept head kh, first pixel p0 of its tile, element offsets of the head's K and Q inside a step's tensors.  (head, tile)
// numbering: the tiles of a head share its K tile out of one L2.  TILE = pixels per workgroup (the host sizes tiles_per_head with it).
struct TapTile {
    int kh, p0;
    int64_t k_off, q_off;
};
template <int TILE> __device__ __forceinline__ TapTile tap_tile_decode(const TapLayer& lay, int wg)
{
    TapTile t;
    const int rel = wg - lay.wg_begin;
    t.kh = rel / lay.tiles_per_head;
    t.p0 = (rel - t.kh * lay.tiles_per_head) * TILE;
    const int bh = lay.bh_first + t.kh;
    const int b = bh / lay.heads, hd = bh - b * lay.heads;
    t.k_off = b * lay.k_sb + hd * lay.k_sh;
    t.q_off = b * lay.q_sb + hd * lay.q_sh;
    return t;
}

// K rows 77..79 (never written by a step; the DMA form re-reads row 76 into them: finite, their logits are masked) must be finite:
// zero them once, both buffers
template <int NT> __device__ __forceinline__ void tap64_zero_pad_rows(unsigned char* kbuf, int tid)
{
    for (int i = tid; i < 2 * 3 * (kTapRow / 16); i += NT) {
        const int buf = i / (3 * (kTapRow / 16)), r = i % (3 * (kTapRow / 16));
        *reinterpret_cast<float4v*>(kbuf + buf * kTapKBuf + kTok * kTapRow + r * 16) = float4v{0, 0, 0, 0};
    }
}

// ---- fetch: LDS-DMA of a step's K and Q rows ------------------------------------------------------------------------------------------
// K: 1 KiB block blk = WAVES j2 + wave (10 blocks: rows 8 blk .. 8 blk + 7; rows 77..79 re-read row 76: finite, their logits are
// masked); lane -> row 8 blk + (lane >> 3), LDS chunk slot lane & 7 = source chunk (lane & 7) ^ ((row >> 1) & 7): the swizzle is applied
// to the SOURCE address, the LDS image of a wave-instruction is lane-linear.  Q: block i = rows 8 i .. 8 i + 7 of the wave's 32, same
// rule.  `wave` is a readfirstlane of tid >> 6: the block choice must stay a scalar branch, not become exec masks.  Every offset is a
// 32-bit byte offset: the tap_*_supported() predicates keep them below 2^31.  The per-lane sources kd_src / qd_src and the Q block
// steps q_s are set up in each kernel (text there: see below).
// the K rows of tensor `kp` (+ scalar byte offset `base`) into the K image at `dst`.  COUNTED (the counted-wait protocol): a block that
// every wave / no wave has is decided at compile time, so that one scalar branch per step remains
template <int WAVES, bool COUNTED = false>
__device__ __forceinline__ void tap64_dma_k(const void* kp, unsigned base, unsigned char* dst, int wave, const unsigned (&kd_src)[3])
{
    const __amdgpu_buffer_rsrc_t kt = tap_tensor_rsrc(kp);
#pragma unroll
    for (int j2 = 0; j2 < 3; ++j2) {
        const int blk = WAVES * j2 + wave;                    // wave-uniform
        const bool every = COUNTED && WAVES * j2 + WAVES - 1 < 10, none = COUNTED && WAVES * j2 >= 10;   // constants once unrolled
        if (every || (!none && blk < 10))
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kt, (lds_ptr_t)(dst + blk * 1024), 16, kd_src[j2], base, 0, 0);
    }
}
// the wave's 32 Q rows of tensor `qp` into its tile
__device__ __forceinline__ void tap64_dma_q(const void* qp, unsigned char* qtile, const unsigned (&qd_src)[2], const unsigned (&q_s)[4])
{
    const __amdgpu_buffer_rsrc_t qt = tap_tensor_rsrc(qp);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(qt, (lds_ptr_t)(qtile + i * 1024), 16, qd_src[i & 1], q_s[i], 0, 0);
}

// ---- MFMA chain ----------------------------------------------------------------------------------------------------------------------
// logits of one K image `kb` over a step's Q operands, the wave's two 16-pixel groups (q0x / q1x; k-steps 0 / 1): five token tiles,
// a0 . q00 -> a1 . q01 per group; tokens 77..79 (tile 4) start their chain from cmask (premask_tile4): -inf
template <typename IN>
__device__ __forceinline__ void tap64_mfma_chain(const unsigned char* kb, int f_rd, const half8& q00, const half8& q01, const half8& q10,
                                                 const half8& q11, const floatx4& cmask, floatx4 (&c0)[5], floatx4 (&c1)[5])
{
#pragma unroll
    for (int mt = 0; mt < 5; ++mt) {
        const half8 a0 = *reinterpret_cast<const half8*>(kb + mt * 16 * kTapRow + f_rd);
        const half8 a1 = *reinterpret_cast<const half8*>(kb + mt * 16 * kTapRow + (f_rd ^ 64));
        c0[mt] = IN::mfma(a0, q00, mt == 4 ? cmask : floatx4{0, 0, 0, 0});
        c1[mt] = IN::mfma(a0, q10, mt == 4 ? cmask : floatx4{0, 0, 0, 0});
        c0[mt] = IN::mfma(a1, q01, c0[mt]);
        c1[mt] = IN::mfma(a1, q11, c1[mt]);
    }
}

// ---- softmax dispatch ----------------------------------------------------------------------------------------------------------------
// softmax + accumulate of one 16-pixel group in the pipeline dtype of IN (bf16 has one softmax flavour); the chain started premasked
template <typename IN, typename ACC_T, bool FAST_EXP>
__device__ __forceinline__ void tap_softmax_accumulate(const floatx4 (&c)[5], const TapLayer& lay, int h, typename Pair<ACC_T>::T (&run)[kSlots16 / 2])
{
    if constexpr (IN::kBf16) softmax20_accumulate_bf16<ACC_T, true>(c, lay, h, run);
    else softmax20_accumulate<ACC_T, FAST_EXP, true>(c, lay, h, run);
}

}  // namespace daam
