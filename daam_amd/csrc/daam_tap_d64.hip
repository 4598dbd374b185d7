// fp16 tap for head_dim <= 64 (64: every SDXL / SD-2.x layer; 40: the 64x64 layers of SD-v1.5, zero-padded
// to 64), gfx950, built on v_mfma_f32_16x16x32_f16.
//
// Why a second tiling: with 32x32 MFMA tiles a lane owns one pixel and 40 token slots, so the
// softmax state (logits, exponentials, running sums) plus three 16-register accumulator tiles push
// the kernel to 160+ VGPRs = 3 waves per SIMD, and the phase timers show the kernel is latency /
// occupancy bound there (VALU ~50 % busy).  With 16x16 tiles the 77 tokens of a pixel are spread
// over FOUR lanes (20 slots each), the live softmax state per 16-pixel group halves, and a wave
// processes its 32 pixels as two groups whose MFMA and softmax phases interleave: 4 waves per SIMD.
//
// Same arithmetic / rounding points as daam_tap_mfma.hip:
//   logits = fp16(f32(q.k) * scale) -> f32 softmax -> fp16(p) -> acc += p (accumulator dtype).
//
// Workgroup = 4 waves = 128 pixels of one (layer, kept head) -- or, for head_dim-64 launches with fp16 sums since round 4, 8 waves = 256
// pixels sharing ONE K tile (template parameter WAVES); wave w: pixels
// [32w, 32w+32) = groups 0 / 1 of 16.  "Swapped" product S^T = K Q^T: A = K rows (lane: token row
// l&15 of the 16-row tile, k = 8*(l>>4)..+7 of the 32-wide k-step), B = Q^T (lane: pixel l&15, same
// k split).  C/D: lane holds pixel l&15 and tokens 16*mt + 4*(l>>4) + r (mt = 0..4, r = 0..3) = 20 slots.
// Both operands reach the MFMAs through LDS in FULL 128-byte rows: K of a step as [80 rows][128 B],
// double-buffered; Q of a step as a wave-private [32 pixel rows][128 B] tile.  Either is fetched from
// HBM one step ahead by coalesced loads (eight consecutive lanes = one whole row) -- straight into LDS by LDS-DMA for
// head_dim 64 (round 3), through staging registers otherwise -- with its 16-byte chunks XOR-swizzled by (row >> 1) & 7,
// which makes the operand reads
// (16 rows x one chunk per ds_read_b128) conflict-free without padding.  Round 2 fetched Q straight into
// the MFMA layout (16 rows x 64 B per load instruction): the same bytes, but 16 bytes per L1 tag
// lookup -- 0.67 lookups per cycle per CU and a read-tag-conflict stall in 20 % of the cycles
// (TCP_TOTAL_CACHE_ACCESSES, TCP_READ_TAGCONFLICT_STALL_CYCLES; profiles/r02_tap_tcp.txt).
#include "daam_tap16_softmax.h"
#include "daam_tap_tile64.h"
#include "daam_tap_rows.h"

// Data path of the head_dim-64 launches (FULL64: every SDXL / SD-2.x layer), as measured over rounds 1-5 (LABNOTES): K and Q go HBM -> LDS by
// LDS-DMA (buffer_load ... lds: the swizzle is applied to the SOURCE address, the LDS image of a wave-instruction is lane-linear) instead of
// through staging registers + ds_write_b128 (24 VGPRs fewer per lane-step); the next step's DMAs go out AHEAD of this step's MFMAs (K right
// after the barrier, Q once the wave's four operand reads have returned); EIGHT waves per workgroup share ONE K tile (256 pixels of a head:
// half the K traffic per pixel; two workgroups per CU = the same 4 waves per SIMD, 53 KB of LDS each).  head_dim < 64 (zero-padded chunks
// cannot come from a DMA) takes the register-staged form on four waves.  The forms that were measured and dropped -- register-staged FULL64,
// DMAs behind the MFMAs, four-wave FULL64, a second Q buffer two steps ahead, head-minor numbering, TLB touches, non-temporal Q, the timing
// ablations -- live as patches under tools/exp/patches/ (tools/exp/build_variant.sh --lab), not in this file.

namespace daam {

// WAVES = waves per workgroup: 4 (128 pixels) or 8 (256 pixels of one head, ONE K tile for twice the pixels)
template <typename ACC_T, int WAVES = 4> constexpr size_t tap_d64_lds_bytes() {
    const size_t kb = 2 * (size_t)kTapKBuf + WAVES * (size_t)kTapQTile, st = (size_t)kTok * (32 * WAVES) * sizeof(ACC_T);
    return (kb > st ? kb : st) + (size_t)kMaxStepsPerLaunch * 2 * sizeof(void*);     // fp16 sums: 37888 -> 4 workgroups per CU
}

// FULL64: every layer of the launch has head_dim == 64 (SDXL): the zero-padding selects of the head_dim < 64 case (8 VALU per
// wave-step) are compiled out
//
// Step protocol of the FULL64 launches (COUNTED; K double-buffered and shared by the workgroup, Q single-buffered and WAVE-PRIVATE; one raw
// s_barrier per step and counted waits -- a __syncthreads() would drain the DMAs, Q included):
//   DMA K(s + 1) -> the other K buffer                               (NK = one to three per wave; an L2 hit with a whole step to land)
//   vmcnt(NK)                 this wave's Q(s) is in LDS: its four DMAs went out BEFORE these K DMAs and vmcnt retires in order
//   Q operands -> registers; lgkmcnt(0); DMA Q(s + 1) -> the Q tile  (in flight for the rest of the step and across the barrier)
//   K operands + MFMAs; softmax + accumulate
//   vmcnt(4), lgkmcnt(0), barrier
// The barrier orders two things, and Q is neither of them:
//   (i)  every wave has finished reading K(s) before the DMAs of K(s + 2) overwrite its buffer: the K operand reads of step s are waited
//        for by the MFMAs that consume them (and by the lgkmcnt(0) in front of the barrier), and K(s + 2) is requested behind the barrier;
//   (ii) every wave's pieces of K(s + 1) have landed before anyone reads them: vmcnt(4) leaves only the four younger Q(s + 1) DMAs
//        outstanding, so this wave's K(s + 1) DMAs are complete when it arrives at the barrier, and the reads are behind it.
// A wave's Q tile is read and refilled by that wave alone: Q(s + 1) is requested once the four operand reads of Q(s) have returned
// (lgkmcnt(0)) and waited for at the top of step s + 1 -- a late Q fetch holds up the wave that owns it, not the workgroup.
// The prologue ends with the same vmcnt(4) + barrier (K(0) is in LDS), the launch with vmcnt(0) + barrier before the staging tile
// reuses the space.  COUNTED = false is the protocol before it: vmcnt(0) at the end of a step (K AND Q), __syncthreads() at the start of
// the next (DAAM_TAP_SYNC=0; the register-staged head_dim < 64 form always).
// (the body is daam_tap_d64_body.inc: one text, two kernel templates, so that the machine code of the earlier protocol stays what it was;
// the parts of the tile that walk / pair / chunk share with it are daam_tap_tile64.h)
#define DAAM_TAP_D64_BOUNDS __launch_bounds__(64 * WAVES, ((WAVES == 8 || (sizeof(ACC_T) == 2 && !IN::kBf16)) ? 4 : 3))

// the protocol before the counted waits (DAAM_TAP_SYNC=0) and the register-staged head_dim < 64 form
template <typename IN, typename ACC_T, bool FAST_EXP, bool FULL64, int WAVES = 4>
__global__ DAAM_TAP_D64_BOUNDS void tap_d64_kernel(const TapLaunch L)
{
    constexpr bool COUNTED = false;
#include "daam_tap_d64_body.inc"
}

// head_dim-64 launches, counted waits (the default): the same kernel name with one more template argument
template <typename IN, typename ACC_T, bool FAST_EXP, bool FULL64, int WAVES, bool COUNTED>
__global__ DAAM_TAP_D64_BOUNDS void tap_d64_kernel(const TapLaunch L)
{
    static_assert(COUNTED && FULL64, "the six-argument form is the counted-wait protocol");
#include "daam_tap_d64_body.inc"
}

bool tap_d64_supported(const DaamQKDesc& d, const void* q, const void* k)
{
    if (d.head_dim < 8 || d.head_dim > 64 || d.head_dim % 8 != 0) return false;
    if (d.k_stride_t * 77 >= (int64_t)1 << 30) return false;   // K element offsets are kept in 32 bits
    return tap_rows_16b(d, q, k, false);
}

template <typename IN, typename ACC_T, bool FAST, bool FULL64, int WAVES = 4, bool COUNTED = false>
static hipError_t launch_d64_k(const TapLaunch& L, hipStream_t stream, int grid, size_t lds)
{
    void (*kernel)(const TapLaunch);
    if constexpr (COUNTED) kernel = tap_d64_kernel<IN, ACC_T, FAST, FULL64, WAVES, true>;
    else kernel = tap_d64_kernel<IN, ACC_T, FAST, FULL64, WAVES>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WAVES), lds, stream, L);
    return hipGetLastError();
}

// counted: the step protocol of the head_dim-64 (DMA) launches, 1 = counted waits + one raw barrier, 0 = vmcnt(0) + __syncthreads()
template <typename IN, typename ACC_T, bool FAST>
static hipError_t launch_d64(const TapLaunch& L, hipStream_t stream, int grid, size_t* lds_out, bool full64, int waves8, bool counted)
{
    if (waves8 && full64) {                                   // every dtype pair fits 128 VGPRs (101-128), no spills
        const size_t lds8 = tap_d64_lds_bytes<ACC_T, 8>();
        *lds_out = lds8;
        return counted ? launch_d64_k<IN, ACC_T, FAST, true, 8, true>(L, stream, grid, lds8) : launch_d64_k<IN, ACC_T, FAST, true, 8>(L, stream, grid, lds8);
    }
    if (waves8) return hipErrorInvalidValue;                  // the host sized the tiles for eight waves: no other form may run them
    const size_t lds = tap_d64_lds_bytes<ACC_T>();
    *lds_out = lds;
    if (!full64) return launch_d64_k<IN, ACC_T, FAST, false>(L, stream, grid, lds);
    return counted ? launch_d64_k<IN, ACC_T, FAST, true, 4, true>(L, stream, grid, lds) : launch_d64_k<IN, ACC_T, FAST, true>(L, stream, grid, lds);
}

// tile pixels the host must size a head_dim-64 launch for: 256 when the eight-wave form takes it (every layer head_dim 64; fp16 Q / K
// with fp16 or f32 sums, bf16 Q / K with bf16 or f32 sums), else 128
int tap_d64_tile_pixels(int in_dtype, int acc_dtype, int full64)
{
    return (tap_tile64_has_waves8(in_dtype, acc_dtype) && full64) ? 256 : 128;
}

bool tap_d64_has_waves8(int in_dtype, int acc_dtype) { return tap_tile64_has_waves8(in_dtype, acc_dtype); }

hipError_t launch_tap_d64(const TapLaunch& L, int in_dtype, int acc_dtype, int fast_exp, int full64, int waves8, int counted, hipStream_t stream, int* grid_out, int* lds_out)
{
    const bool cw = counted != 0;
    const int grid = L.wgs_per_xcd * 8;
    *grid_out = grid;
    size_t lds = 0;
    hipError_t e;
    if (in_dtype == 2) {                                       // bf16 pipeline: one softmax flavour
        if (acc_dtype == 2) e = launch_d64<InBF16, bf16_t, true>(L, stream, grid, &lds, full64 != 0, waves8, cw);
        else if (acc_dtype == 1) e = launch_d64<InBF16, float, true>(L, stream, grid, &lds, full64 != 0, waves8, cw);
        else return hipErrorInvalidValue;
    } else if (acc_dtype != 0 && acc_dtype != 1) {
        return hipErrorInvalidValue;
    } else if (fast_exp) {
        e = acc_dtype == 0 ? launch_d64<InF16, _Float16, true>(L, stream, grid, &lds, full64 != 0, waves8, cw) : launch_d64<InF16, float, true>(L, stream, grid, &lds, full64 != 0, waves8, cw);
    } else {
        e = acc_dtype == 0 ? launch_d64<InF16, _Float16, false>(L, stream, grid, &lds, full64 != 0, waves8, cw) : launch_d64<InF16, float, false>(L, stream, grid, &lds, full64 != 0, waves8, cw);
    }
    *lds_out = (int)lds;
    return e;
}

}  // namespace daam
