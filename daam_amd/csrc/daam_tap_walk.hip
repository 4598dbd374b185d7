// Window-walking head_dim-64 tap (time windows): one workgroup owns a (layer, kept head, 256-pixel tile) and walks the
// layer's time windows in recorded order inside ONE launch -- per window: zero (or load) the register sums, run the window's steps,
// write the sums to the window's slice, go on.  tap_d64_kernel runs one workgroup per (window, head, tile): with one window per
// denoising step every chain is one step long, its step-ahead prefetch has nothing to prefetch and the launch has 50 times the
// workgroups.  Here the fetch pipeline does not stop at a window boundary: the entry's step pointers (every window's) are staged in
// LDS once, and the K / Q tiles of the first step of window w + 1 are requested during the last step of window w, exactly as inside
// a chain; the redundant re-fetch of "the last step" happens once, at the end of the entry.
//
// Every window's sums are bit-identical to tap_d64_kernel<IN, ACC_T, FAST, true, 8> run on that window's steps alone: the same
// tile (daam_tap_tile64.h: geometry, swizzle, descriptor, prologue, MFMA chain, softmax dispatch; eight waves, 256 pixels of one kept
// head, one K tile for all of them), acc = acc + p in the accumulator dtype.  This file adds the window loop and its own staging.
//
// The write-back of a window happens while the next step's tiles already sit in the K buffer / the Q tiles, so the staging tile
// cannot alias them as it does in tap_d64_kernel: it has LDS of its own and takes the 256 pixels in passes of 128 (2-byte sums) or
// 64 (f32 sums) -- 19.25 KiB either way.  LDS: 2 K buffers (20 KiB) + 8 Q tiles (32 KiB) + staging (19.25 KiB) + step pointers
// (1 KiB) = 72.25 KiB: two workgroups per CU, four waves per SIMD at <= 128 VGPRs, like tap_d64_kernel.
#include "daam_tap16_softmax.h"
#include "daam_tap_tile64.h"
#include "daam_tap_walk.h"

namespace daam {
namespace tap_walk {

constexpr int kWaves = 8;
constexpr int kStageOff = kTapQOff + kWaves * kTapQTile;   // behind the tile's K buffers and Q tiles: the write-back staging tile [kTok][stage pixels]
constexpr int kStageBytes = kTok * 256;             // 128 pixels x 2 bytes = 64 pixels x 4 bytes per token row
constexpr int kPtrOff = kStageOff + kStageBytes;    // then the entry's step pointers
constexpr size_t kLdsBytes = (size_t)kPtrOff + (size_t)kMaxStepsPerLaunch * 2 * sizeof(void*);
static_assert(kLdsBytes <= 80 * 1024, "two workgroups per CU");

// one running-sum element from global memory (the non-fresh first window of an entry: a window cut by a launch boundary)
template <typename ACC_T> __device__ __forceinline__ ACC_T load_acc(const ACC_T* p, unsigned i) {
    if constexpr (sizeof(ACC_T) == 2) return __builtin_bit_cast(ACC_T, as_global<unsigned short>(p)[i]);
    else return as_global<float>(p)[i];
}

// The lane id, computed afresh where it is asked for.  The load and write-back code of a window derives its lane coordinates from it
// instead of from values computed at kernel start: nothing of their address arithmetic is then hoisted ahead of the window loop and
// kept in registers across the steps (the step body leaves none to spare: that cost spills).
__device__ __forceinline__ int walk_lane_id() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

}  // namespace tap_walk

template <typename IN, typename ACC_T, bool FAST_EXP>
__global__ __launch_bounds__(512, 4) void tap_walk_kernel(const WalkLaunch W)
{
    using namespace tap_walk;
    constexpr int NT = 64 * kWaves;
    constexpr int TILE = 32 * kWaves;
    constexpr int VEC = AccVec<ACC_T>::kPerVec;
    constexpr int CH = kStageBytes / kTok / (int)sizeof(ACC_T);   // pixels per write-back pass: 128 / 64
    constexpr int PASSES = TILE / CH, WPP = CH / 32;              // waves whose pixels one pass covers
    constexpr int PPR = CH / VEC;                                 // 16-byte pieces per staged row (16)

    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* kbuf = smem;                               // [2][kTapKBuf], then the eight waves' Q tiles
    ACC_T* stage = reinterpret_cast<ACC_T*>(smem + kStageOff);    // [kTok][CH]: aliases nothing
    const void** sptr = reinterpret_cast<const void**>(smem + kPtrOff);

    const TapLaunch& L = W.L;
    const int wg = mfma_logical_block(L.total_wgs, L.wgs_per_xcd);
    if (wg < 0) return;
    tap_mark_started(L);
    const DAAM_GLOBAL TapLayer* gl = as_global<TapLayer>(L.layers);
    const int li = mfma_find_layer(gl, L.n_layers, wg);
    TapLayer lay;
    load_layer(gl + li, &lay);
    const DAAM_GLOBAL WalkEntry* ent = as_global<WalkEntry>(W.entries) + li;
    const int n_win = ent->n_win;
    const DAAM_GLOBAL WalkWin* wins = as_global<WalkWin>(W.wins) + ent->win_begin;
    const int tid = threadIdx.x;
    tap_step_ptrs_to_lds<NT>(L, lay, true, sptr, tid);        // every window's steps, once
    const int n_steps = lay.n_steps;                          // of the whole entry
    const int rel = wg - lay.wg_begin;
    // (the quotient comes off the VALU: as scalars, head and tile do not turn every window's sum address into a per-lane 64-bit value)
    const int kh = __builtin_amdgcn_readfirstlane(rel / lay.tiles_per_head);
    const int p0 = __builtin_amdgcn_readfirstlane((rel - kh * lay.tiles_per_head) * TILE);
    const int bh = lay.bh_first + kh;
    const int b = bh / lay.heads, hd = bh - b * lay.heads;
    const int64_t k_off = b * lay.k_sb + hd * lay.k_sh;
    const int64_t q_off = b * lay.q_sb + hd * lay.q_sh;

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, h = lane >> 4;

    tap64_zero_pad_rows<NT>(kbuf, tid);
    __syncthreads();                                          // sptr visible

    // fetch addressing: the LDS-DMA form (daam_tap_tile64.h).  The source set-up and the K issue are text here: as functions of the
    // header they change every instance (set-up 16 bytes shorter, K issue 4 bytes longer, q_s rescheduled; same registers)
    const unsigned k_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(k_off * 2));
    const int q_rows_in = __builtin_amdgcn_readfirstlane(lay.hw - (p0 + wave * 32));
    const unsigned q_step8 = (unsigned)__builtin_amdgcn_readfirstlane(8 * (int)lay.q_sp * 2);   // bytes per 8 pixel rows
    unsigned q_s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q_s[i] = 8 * i < q_rows_in ? (unsigned)i * q_step8 : 0u;
    unsigned char* qtile = kbuf + kTapQOff + wave * kTapQTile;
    const int f_rd = j * kTapRow + swz_chunk(j, h);           // k-step 1: ^ 64
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
    auto dma_k = [&](int s, int buf) {
        const __amdgpu_buffer_rsrc_t kt = tap_tensor_rsrc(sptr[2 * s + 1]);
#pragma unroll
        for (int j2 = 0; j2 < 3; ++j2) {
            const int blk = kWaves * j2 + wave;               // wave-uniform
            if (blk < 10)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(kt, (lds_ptr_t)(kbuf + buf * kTapKBuf + blk * 1024), 16, kd_src[j2], k_base, 0, 0);
        }
    };
    auto dma_q = [&](int s) { tap64_dma_q(sptr[2 * s], qtile, qd_src, q_s); };
    const floatx4 cmask = premask_tile4(h);
    typename Pair<ACC_T>::T run0[kSlots16 / 2], run1[kSlots16 / 2];   // slot pairs (2i, 2i+1)
    // step g of the ENTRY (the windows' steps numbered through): tap_d64_kernel's step body; the fetches of step g + 1 go out whether
    // or not it belongs to the same window
    auto step = [&](int g) {
        __syncthreads();
        const unsigned char* kb = kbuf + (g & 1) * kTapKBuf;
        const int g_fetch = min(g + 1, n_steps - 1);          // branch-free: the entry's last step re-fetches itself
        dma_k(g_fetch, (g + 1) & 1);
        const half8 q00 = *reinterpret_cast<const half8*>(qtile + f_rd), q01 = *reinterpret_cast<const half8*>(qtile + (f_rd ^ 64));
        const half8 q10 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + f_rd);
        const half8 q11 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + (f_rd ^ 64));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dma_q(g_fetch);
        floatx4 c0[5], c1[5];
        tap64_mfma_chain<IN>(kb, f_rd, q00, q01, q10, q11, cmask, c0, c1);
        tap_softmax_accumulate<IN, ACC_T, FAST_EXP>(c0, lay, h, run0);
        tap_softmax_accumulate<IN, ACC_T, FAST_EXP>(c1, lay, h, run1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's DMAs have landed; the next step's barrier publishes K
    };
    dma_k(0, 0);
    dma_q(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    const int hw = __builtin_amdgcn_readfirstlane(lay.hw);    // scalar for the window code below
    int g = 0;
    void* win_acc = wins[0].acc;
    int wn = wins[0].n_steps, win_fresh = wins[0].fresh;
    for (int w = 0; w < n_win; ++w) {
        ACC_T* acc = reinterpret_cast<ACC_T*>(win_acc) + (size_t)kh * kTok * hw;
        const int n_here = wn, fresh = win_fresh;
        const int wnext = min(w + 1, n_win - 1);              // the next window's record arrives during this window's steps
        win_acc = wins[wnext].acc;
        wn = wins[wnext].n_steps;
        win_fresh = wins[wnext].fresh;
        // ---- the window's sums -> registers: zero, or (a window a launch boundary cut) straight from memory ----
        if (!fresh) {
            // the lane's coordinates come from a fresh lane id (see walk_lane_id); its pixels of groups 0 / 1 and its token slots are
            // clamped into the layer (kTok * hw < 2^31), and what lies outside stays zero
            const int lw = walk_lane_id(), jw = lw & 15, hq = lw >> 4;
            const int px0 = p0 + wave * 32 + jw, px1 = px0 + 16;
            const unsigned c0 = (unsigned)min(px0, hw - 1), c1 = (unsigned)min(px1, hw - 1);
#pragma unroll
            for (int i = 0; i < kSlots16; ++i) {
                const int t = slot16_token(i, hq);
                const unsigned row = (unsigned)(min(t, kTok - 1) * hw);
                const ACC_T v0 = load_acc(acc, row + c0), v1 = load_acc(acc, row + c1);
                run0[i >> 1][i & 1] = (t < kTok && px0 < hw) ? from_acc<ACC_T>(v0) : 0;
                run1[i >> 1][i & 1] = (t < kTok && px1 < hw) ? from_acc<ACC_T>(v1) : 0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kSlots16; ++i) { run0[i >> 1][i & 1] = 0; run1[i >> 1][i & 1] = 0; }
        }
        for (int s = 0; s < n_here; ++s, ++g) step(g);
        // ---- write back: registers -> staging [token][pixel] -> 16-byte row pieces, CH pixels per pass.  The K buffer and the Q
        // tiles hold the next window's first step by now: the staging tile is LDS of its own ----
        const int lw = walk_lane_id(), jw = lw & 15, hq = lw >> 4, tw = wave * 64 + lw;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            if (p0 + p * CH >= hw) break;                     // workgroup-uniform: the tile ends before this pass
            if (wave / WPP == p) {
                const int col = (wave % WPP) * 32;
#pragma unroll
                for (int i = 0; i < kSlots16; ++i) {
                    const int t = slot16_token(i, hq);
                    if (t < kTok) {
                        stage[t * CH + col + jw] = to_acc<ACC_T>(run0[i >> 1][i & 1]);
                        stage[t * CH + col + 16 + jw] = to_acc<ACC_T>(run1[i >> 1][i & 1]);
                    }
                }
            }
            __syncthreads();
            for (int piece = tw; piece < kTok * PPR; piece += NT) {
                const int row = piece / PPR, col = (piece - row * PPR) * VEC;
                if (p0 + p * CH + col < hw)
                    *as_global_rw<float4v>(acc + (size_t)row * hw + p0 + p * CH + col) =
                        *reinterpret_cast<const float4v*>(stage + row * CH + col);
            }
            __syncthreads();                                  // the pieces are read before the next pass / window stages again
        }
    }
}

int tap_walk_tile_pixels() { return 32 * tap_walk::kWaves; }

template <typename IN, typename ACC_T, bool FAST>
static hipError_t launch_walk(const WalkLaunch& W, hipStream_t stream, int grid)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tap_walk_kernel<IN, ACC_T, FAST>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)tap_walk::kLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((tap_walk_kernel<IN, ACC_T, FAST>), dim3(grid), dim3(512), tap_walk::kLdsBytes, stream, W);
    return hipGetLastError();
}

hipError_t launch_tap_walk(const WalkLaunch& W, int in_dtype, int acc_dtype, int fast_exp, hipStream_t stream, int* grid_out, int* lds_out)
{
    if (!W.L.layers || !W.entries || !W.wins || !tap_tile64_has_waves8(in_dtype, acc_dtype)) return hipErrorInvalidValue;
    const int grid = W.L.wgs_per_xcd * 8;
    *grid_out = grid;
    *lds_out = (int)tap_walk::kLdsBytes;
    if (in_dtype == 2)                                         // bf16 pipeline: one softmax flavour
        return acc_dtype == 2 ? launch_walk<InBF16, bf16_t, true>(W, stream, grid) : launch_walk<InBF16, float, true>(W, stream, grid);
    if (fast_exp)
        return acc_dtype == 0 ? launch_walk<InF16, _Float16, true>(W, stream, grid) : launch_walk<InF16, float, true>(W, stream, grid);
    return acc_dtype == 0 ? launch_walk<InF16, _Float16, false>(W, stream, grid) : launch_walk<InF16, float, false>(W, stream, grid);
}

}  // namespace daam
