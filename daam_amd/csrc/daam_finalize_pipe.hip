// x2 (32 -> 64) finalize of fp16 planes, software-pipelined (round 3): compute_global_heat_map's per-key
// bicubic -> clamp(min=0) -> mean (reference daam/trace.py:112-126) for every 32 x 32 key of a selection.
//
// Same arithmetic as finalize_up32_mfma_kernel (daam_finalize.hip: both bicubic passes on v_mfma_f32_32x32x16_f16, T as an
// fp16 hi + lo pair, clamp + accumulate as ONE v_max_i32 on the result of an MFMA chain that starts from the running sums),
// rebuilt around what bounded that kernel -- 630 cycles per half plane at 4 waves per SIMD although its own instruction stream
// runs in 418, and in 358-380 when the stages of consecutive planes overlap (tools/gen_ubench_fin.py):
//   * TWO waves per SIMD, each running a hand-scheduled two-deep software pipeline (tools/gen_fin_pipe.py ->
//     daam_finalize_pipe_asm.inc, one asm statement): the pass-2 MFMAs of plane i, the clamps of plane i-1, the hi / lo split
//     of plane i+1 and the pass-1 MFMAs of plane i+2 are in flight together, every VALU instruction sits in a fixed gap behind
//     an MFMA that does not depend on it, results alternate between two register sets (even / odd planes; summed at the end);
//   * planes reach the MFMAs through an LDS ring of 8 planes per workgroup filled by LDS-DMA (global_load_lds_dwordx4: each of
//     the two waves fetches one 1 KiB half of every plane and both read all of it; counted vmcnt + one s_barrier per plane, no
//     staging registers): a plane crosses L2 -> LDS once (wave-private rings fetched every plane twice: 6.7 TB/s of traffic,
//     the bound of the first version), 7 planes in flight per workgroup;
//   * workgroup = 2 waves = the two 32-column halves (nt) of the output for ONE (token, key chunk); a wave walks ALL keys of its
//     chunk from a host-built pointer table padded with an all-zero plane to a common even length (no per-wave remainder code,
//     no key cap);
//   * the same-size (64 x 64) keys of the selection ride along: every wave adds its share of them to the same accumulators with an
//     identity MFMA + the same one-v_max clamp BEFORE entering the loop, under the latency of the ring's first planes -- SDXL-1024's
//     finalize is ONE class kernel (a second kernel on a second stream cost 15 us of event fork / join per call);
//   * ~215 VGPRs -> 2 waves per SIMD.
//
// Round 6: the same pipeline for the other two dtypes a context's sums can have (the reference's finalize takes whatever the running
// sums are, daam/trace.py:111-116) -- the generator writes one schedule per dtype:
//   * bf16 planes: pass 1 on v_mfma_f32_32x32x16_bf16 -- the plane is its A operand as it is; the tap matrix is NOT a bf16 matrix (three taps
//     clamped onto a border column add up to 283/256: nine significant bits), so the host splits W = W' + E into two bf16 matrices (E = 1/256
//     at [0][0] and [63][31]) and pass 1 has a third MFMA whose A operand -- plane columns 0..7 | 24..31 -- is selected from the two pieces
//     the lane holds anyway (4 v_cndmask): 11 MFMAs per plane.  T, pass 2, clamp and the folded same-size keys (identity MFMA in bf16) as above;
//   * f32 planes (accumulate='float32'): 4 KiB per plane, ring of 8; a lane reads its A pieces as 16 floats and splits them into an
//     fp16 hi + lo pair exactly like pass 2 splits T (2^-22 relative for |v| >= 2^-3, an absolute 2^-25 below that, where lo is an fp16
//     subnormal, inf above 65504 -- the same error and the same domain pass 2 already has, see daam_finalize.hip): 4 pass-1 MFMAs and 32 more
//     VALU instructions per plane.  The 16-byte pieces of a 128-byte plane row sit XOR-swizzled in the ring (piece ^ ((row >> 1) & 7), done
//     on the DMA's per-lane SOURCE address): the four ds_read_b128 of an A operand are conflict-free.  The folded same-size keys take the
//     VALU (every lane loads the elements it owns in the C/D layout, acc += max(P, 0)).
#include "daam_finalize.h"

namespace daam {

constexpr int kPipeRing = 16;              // planes per workgroup ring (the generated schedule is per depth: tools/gen_fin_pipe.py)
constexpr int kSameBatch = 8;           // same-size keys whose pieces are fetched together (32 loads in flight per lane)
constexpr int kSameBatchF32 = 4;        // ... of f32 planes (128 dword loads in flight per lane)
constexpr int kPipePlane = 32 * 32 * 2; // bytes

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// DT = plane dtype: DAAM_F16, DAAM_BF16, DAAM_F32 (daam_hip.h)
// (2 waves per SIMD: the register budget the allocator must respect -- arch VGPRs + AGPRs <= 256)
template <int DT>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void finalize_up32_pipe_kernel(const FinPipeLaunch L)
{
#include "daam_fin_pipe_kernel_body.inc"
}

// daam_finalize_groups: blockIdx.z = group; the group's chunks start ptr_off / same_off entries into the pointer tables
template <int DT>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void finalize_up32_pipe_grouped_kernel(const FinPipeGroupLaunch G)
{
    const FinGroup& grp = G.g[blockIdx.z];
    if ((int)blockIdx.x >= grp.rows) return;
    FinPipeLaunch L = G.L;
    L.key_ptrs += grp.ptr_off;
    if (L.same_ptrs) L.same_ptrs += grp.same_off;
    L.out += grp.out_off;
    L.tokens = grp.rows;
    L.inv_n = grp.inv_n;
#include "daam_fin_pipe_kernel_body.inc"
}

// G == NULL: the single-map kernel on L; otherwise L is G->L and the grouped form runs on *G with grid z = n_groups
hipError_t launch_finalize_up32_pipe(const FinPipeLaunch& L, const FinPipeGroupLaunch* G, int n_groups, int dtype, hipStream_t stream,
                                     int* grid_out)
{
    const dim3 grid(L.tokens, L.n_chunks, n_groups);
    *grid_out = fin_workgroups(grid);
    return fin_dispatch(dtype, [&](auto t) {
        constexpr int DT = decltype(t)::dt;
        return G ? fin_launch(finalize_up32_pipe_grouped_kernel<DT>, grid, 128, 0, stream, *G) : fin_launch(finalize_up32_pipe_kernel<DT>, grid, 128, 0, stream, L);
    });
}

// planes the ring prefetches past a chunk's last one (pointer-table padding): 16 planes of 2 KiB, 8 of 4 KiB
int finalize_pipe_ring(int dtype) { return dtype == DAAM_F32 ? kPipeRing / 2 : kPipeRing; }

}  // namespace daam

