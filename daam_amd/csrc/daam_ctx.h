// Host-only internals of libdaam_hip.so shared by the parts of the C ABI (daam_api.hip: context, layers, attend, profiling;
// daam_tap_api.hip: the tap entry points; daam_finalize_api.hip: the finalize entry points; daam_epilogue.hip, daam_word_masks.hip,
// daam_mask_matrix.hip, daam_region_scores.hip: the epilogue's, each beside its kernels): the tap and attend kernel files' host
// launchers (the finalize's: daam_finalize.h, daam_fin_rect.h, daam_fin_bins.h), the context and its helpers.
#pragma once
#include "daam_types.h"
#include "daam_finalize.h"
#include "daam_fin_bins.h"
#include "daam_fin_rect.h"

#include <deque>
#include <string>
#include <utility>
#include <vector>

namespace daam {
hipError_t launch_tap_generic(const TapLaunch&, int, int, int, hipStream_t, int*, int*);
hipError_t launch_tap_mfma(const TapLaunch&, int acc_dtype, int max_d, int fast_exp, hipStream_t, int*, int*);
bool tap_mfma_supported(const DaamQKDesc&, const void* q, const void* k);
int tap_mfma_tile_pixels();
int tap_mfma_ksteps(int head_dim);
int tap_mfma_max_steps();
hipError_t launch_tap_d64(const TapLaunch&, int in_dtype, int acc_dtype, int fast_exp, int full64, int waves8, int counted, hipStream_t, int*, int*);
int tap_d64_tile_pixels(int in_dtype, int acc_dtype, int full64);
bool tap_d64_has_waves8(int in_dtype, int acc_dtype);      // the eight-wave form exists for this dtype pair (tap_tile64_has_waves8)
bool tap_wide_supported(const DaamQKDesc&, const void* q, const void* k);
hipError_t launch_tap_wide(const TapLaunch&, int acc_dtype, int max_head_dim, int fast_exp, hipStream_t, int*, int*);
bool tap_d64_supported(const DaamQKDesc&, const void* q, const void* k);
bool tap_chunk_supported(const DaamQKDesc&, const void* q, const void* k);
hipError_t launch_tap_chunk(const TapLaunch&, int in_dtype, int acc_dtype, int fast_exp, int interleave, hipStream_t, int*, int*);
bool tap_slab_supported(const DaamQKDesc&, const void* q, const void* k);
int tap_slab_heads(int head_dim);
int tap_slab_tile_pixels();
hipError_t launch_tap_slab(const TapLaunch&, int acc_dtype, int fast_exp, hipStream_t, int*, int*);
int tap_pair_tile_pixels();
hipError_t launch_tap_pair(const TapLaunch&, int fast_exp, hipStream_t, int*, int*);

hipError_t launch_tap_probs(const ProbsLaunch&, int, int, hipStream_t, int*, int*);
hipError_t launch_upload(void* dst, const void* src_host_mapped, size_t bytes, void* zero, size_t zero_bytes, hipStream_t);
bool attend_d64_supported(int in_dtype, int head_dim, int tokens, const int64_t* strides, int n_strides, const void* const* ptrs, int n_ptrs);
hipError_t launch_attend_d64(const AttendLaunch&, int in_dtype, int acc_dtype, int fast_exp, hipStream_t, int*, int*);
hipError_t launch_clock_monitor(unsigned long long* samples, int n_samples, int period_us, hipStream_t);
hipError_t launch_start_gate(const unsigned* counter, unsigned target, int timeout_us, unsigned* timeouts, hipStream_t);
constexpr int kClockMaxSamples = 4096;
}  // namespace daam

using namespace daam;

// sets the calling thread's daam_last_error() text (defined in daam_api.hip) and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// the end of an entry point that has enqueued its kernels: 0, or fail() with "<what> launch: <the HIP error's text>"
int launched(const char* what, hipError_t e = hipGetLastError());

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) return fail((int)_e, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace daam {

// ---- pinned upload ring -----------------------------------------------------------------
// alloc() hands out a pinned host region and its device twin; commit() copies it H2D on the
// stream with a tiny copy KERNEL that reads the (device-mapped) pinned buffer - hipMemcpyAsync put a
// ~0.2 ms cross-queue bubble between the copy and the consuming kernel - and, after the consuming
// kernel has been enqueued, release() records an event so the region is only reused once that
// kernel has run.  Wrap-around waits (hipEventSynchronize)
// only if the GPU is more than one ring behind the host.
struct Ring {
    static constexpr size_t kBytes = 8u << 20;
    char* host = nullptr;
    char* host_dev = nullptr;         // device-side address of the pinned buffer
    char* dev = nullptr;
    size_t head = 0;                  // next free byte
    struct Busy { size_t begin, end; hipEvent_t ev; };
    std::deque<Busy> busy;
    std::vector<hipEvent_t> pool;

    hipError_t init() {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), kBytes, hipHostMallocMapped);
        if (e != hipSuccess) return e;
        e = hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), host, 0);
        if (e != hipSuccess) return e;
        return hipMalloc(reinterpret_cast<void**>(&dev), kBytes);
    }
    void destroy() {
        for (auto& b : busy) { (void)hipEventSynchronize(b.ev); (void)hipEventDestroy(b.ev); }
        for (auto ev : pool) (void)hipEventDestroy(ev);
        busy.clear(); pool.clear();
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        host = dev = nullptr;
    }
    bool overlaps(size_t b, size_t e) const {
        for (auto& x : busy) if (b < x.end && x.begin < e) return true;
        return false;
    }
    hipError_t alloc(size_t bytes, size_t* off) {
        bytes = (bytes + 255) & ~size_t(255);
        if (bytes > kBytes) return hipErrorOutOfMemory;
        if (head + bytes > kBytes) head = 0;
        // retire finished regions; block on the oldest ones still overlapping the request
        while (!busy.empty() && (hipEventQuery(busy.front().ev) == hipSuccess)) {
            pool.push_back(busy.front().ev);
            busy.pop_front();
        }
        while (overlaps(head, head + bytes)) {
            hipError_t e = hipEventSynchronize(busy.front().ev);
            if (e != hipSuccess) return e;
            pool.push_back(busy.front().ev);
            busy.pop_front();
        }
        *off = head;
        head += bytes;
        cur_begin = *off;
        cur_end = head;
        return hipSuccess;
    }
    size_t cur_begin = 0, cur_end = 0;
    hipError_t commit(size_t off, size_t bytes, hipStream_t s, void* zero = nullptr, size_t zero_bytes = 0) {
        return launch_upload(dev + off, host_dev + off, bytes, zero, zero_bytes, s);
    }
    hipError_t release_range(size_t begin, size_t end, hipStream_t s) {
        cur_begin = begin;
        cur_end = end;
        return release(s);
    }
    hipError_t release(hipStream_t s) {
        hipEvent_t ev;
        if (!pool.empty()) { ev = pool.back(); pool.pop_back(); }
        else {
            hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipEventRecord(ev, s);
        if (e != hipSuccess) return e;
        busy.push_back({cur_begin, cur_end, ev});
        return hipSuccess;
    }
};

struct Layer {
    bool configured = false;
    int heads = 0, side = 0, hw = 0, factor = 0;   // side: h == w, or 0 for a layer of unequal sides
    int h = 0, w = 0;        // hw = h * w, position p = pixel (p / w, p % w)
    int rtab = -2;           // finalize_rect_kernel's table pair of (h, w): -1 = the output's size, -2 = not looked up yet (rect_tab)
    void* acc = nullptr;
    bool owned = false;
    size_t bytes = 0;
    int tab = -1;
    bool dirty = false;      // tapped since the last reset (else the sums are known to be zero)
    bool zero_pending = false;  // reset() was called but the buffer has not been cleared yet: the next
                                // MFMA tap overwrites it (fresh), anything else clears it first
};

struct Pending {
    int layer;
    const void* q;
    const void* k;
    DaamQKDesc d;
};

constexpr int kMaxTabs = 16;
constexpr int kMaxBins = 64;         // time windows of a binned context (daam_ctx_set_time_bins)

}  // namespace daam

struct DaamCtx {
    int device = 0;                    // HIP device the context was created on; every entry point runs there
    int max_layers, tokens, out_side, acc_dtype;   // out_side: out_h == out_w, or 0 for an output of unequal sides
    int out_h = 0, out_w = 0;
    // finalize_rect_kernel: one table pair per distinct (h, w), [kMaxTabs][out_w + out_h][4] (row table, then column table);
    // allocated with the first layer that needs one
    std::vector<std::pair<int, int>> rtab_hw;
    int16_t* d_rtab_idx = nullptr;
    float* d_rtab_w = nullptr;
    // the finalize of this context runs finalize_rect_kernel: the output or a configured layer has unequal sides
    bool rect() const {
        if (out_h != out_w) return true;
        for (const Layer& l : layers)
            if (l.configured && l.h != l.w) return true;
        return false;
    }
    // Layer slots.  Un-binned: slot = layer.  Time-binned (daam_ctx_set_time_bins): slot = window * max_layers + layer, an
    // ordinary Layer over the window's slice of the layer's sums [n_bins][heads, tokens, side, side]; every tap entry point maps
    // (layer, step) to its slot, so the deferred launch chains the steps of one window per table entry (TapLayer) as it
    // chains the steps of a layer without windows.
    std::vector<Layer> layers;
    int n_bins = 0;                    // 0: no windows (daam_ctx_set_time_bins never called)
    int bin_first[kMaxBins] = {0};     // first step of each window
    std::vector<int> tap_steps;        // per layer: taps since daam_reset (the step index of the next tap)
    void* bin_scratch = nullptr;       // daam_finalize_bins: f32 planes of the window-range reduction (grows, never shrinks)
    size_t bin_scratch_bytes = 0;
    int slot_of(int layer) const {
        if (n_bins <= 1) return layer;
        const int step = tap_steps[layer];
        int b = n_bins - 1;
        while (b > 0 && bin_first[b] > step) --b;
        return b * max_layers + layer;
    }
    Ring ring;
    int16_t* d_tab_idx = nullptr;
    float* d_tab_w = nullptr;
    std::vector<int> tab_sides;
    std::vector<int> tab_fp16_exact;   // every (border-merged) tap weight is an fp16 number
    void* d_up32_ops = nullptr;        // finalize_up32_mfma_kernel operands of the 32 -> 64 table (see build_up32_ops)
    void* d_up32_ops_bf16 = nullptr;   // the same for bf16 planes on the pipelined kernel: pass-1 pieces as bf16 bit patterns, W = W' + E (NULL: no such split)
    int up32_tab = -1;
    int no_mfma_finalize = 0;
    int no_fold_same = 0;             // debugging / A-B: the same-size class as its own kernel beside the pipelined one
    int no_pipe_finalize = 0;         // debugging / A-B: the round-2 x2 MFMA kernel instead of the software-pipelined one
    void* d_zero_planes = nullptr;    // [tokens][32 x 32] zeros (sized for f32 planes): padding keys of the pipelined x2 finalize
    int no_paired_finalize = 0;       // debugging / A-B: same-size and x2 class as two launches
    // finalize tables kept on the device between calls: a generation's compute_global_heat_map() selects the same keys at the same
    // addresses as the previous one, so the key / pointer tables are uploaded once and compared on the host afterwards
    static constexpr size_t kFinTabCap = 1u << 20;
    char* d_fin_tab = nullptr;
    std::vector<char> fin_tab_host;   // the bytes d_fin_tab holds (when fin_tab_valid)
    bool fin_tab_valid = false;
    hipStream_t fin_tab_stream = nullptr;   // the stream its upload and its readers were enqueued on
    int no_w8 = 0;                    // debugging / A-B: DAAM_TAP_W8=0 (head_dim-64 launches on 4-wave workgroups of 128 pixels instead of 8-wave / 256)
    int tap_sync = 1;                 // A-B: DAAM_TAP_SYNC=0 (head_dim-64 DMA launches: vmcnt(0) + __syncthreads() per step instead of counted waits + one raw barrier)
    int no_fin_cache = 0;             // debugging / A-B: DAAM_NO_FIN_CACHE=1 (tables through the ring + zeroing in every call)
    // daam_finalize_prepare: the output buffer the next daam_finalize accumulates into has been zeroed already (prep_*), or is to
    // be zeroed by the table-upload kernel of the next tap launch (fold_*)
    float* prep_out = nullptr;
    hipStream_t prep_stream = nullptr;
    int prep_rows = 0;                 // token rows the announced call covers (= the rows that were / will be cleared)
    float* fold_out = nullptr;
    size_t fold_bytes = 0;
    hipStream_t fold_stream = nullptr;
    std::vector<Pending> pending;
    std::vector<int> pending_count;   // per layer: recorded steps
    std::vector<int> pending_last;    // per layer: index of its newest entry in `pending`
    void drop_pending() { pending.clear(); pending_count.clear(); pending_last.clear(); }
    int last_grid[2] = {0, 0}, last_block[2] = {0, 0}, last_lds[2] = {0, 0};
    std::string last_kernels[2];       // daam_last_kernels: what the last tap launch / finalize call launched, '+'-separated
    int last_fin_side = 0;             // finalize class kernels of the last call that ran on auxiliary streams
    int last_flush_kernels = 0, last_flush_side = 0, last_flush_steps = 0;   // daam_last_flush: kernels / of them on side streams / longest step chain
    long long n_flushes = 0;           // tap launches (flushes that launched something) since the context was created
    int profile = 0;
    hipEvent_t prof_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    // daam_profile_enable(ctx, 2): every launch of a kind (0 tap, 1 finalize) gets its own event pair out of a ring, so that a caller
    // can time the launches of a whole timed region WITHOUT synchronising inside it (daam_profile_history afterwards)
    static constexpr int kProfHist = 256;
    std::vector<hipEvent_t> hist_ev[2][2];
    long long hist_count[2] = {0, 0};
    hipEvent_t prof_event(int which, int end) {
        if (profile == 2 && !hist_ev[which][end].empty()) return hist_ev[which][end][(size_t)(hist_count[which] % kProfHist)];
        return prof_ev[which][end];
    }
    // shader-clock monitor (daam_clock_monitor_*): one wave on its own stream samples the shader-cycle counter and the
    // 100 MHz reference counter into pinned memory while the kernels under test run
    unsigned long long* clk_host = nullptr;
    unsigned long long* clk_dev = nullptr;
    int clk_samples = 0;
    hipStream_t clk_stream = nullptr;
    static constexpr int kAux = 3;     // side streams of multi-kind tap flushes (see daam_tap_flush)
    hipStream_t aux_stream[kAux] = {nullptr, nullptr, nullptr};
    hipEvent_t aux_fork = nullptr, aux_join[kAux] = {nullptr, nullptr, nullptr};
    unsigned* d_started = nullptr;     // start gate of multi-kernel flushes: workgroups of side kernels started so far (wraps)
    unsigned started_target = 0;       // ... and how many the host has launched
    unsigned* gate_timeouts = nullptr; // pinned, device-mapped: gates that gave up after their 200 us (the side kernels were NOT running beside them)
    unsigned* gate_timeouts_dev = nullptr;
    int no_start_gate = 0;             // DAAM_NO_START_GATE=1 (debugging / A-B), or a failed flush left counter and target in disagreement
    unsigned gate_timeouts_seen = 0;   // value of *gate_timeouts when the gate was last armed
    unsigned long long gate_enqueued = 0;   // gated flushes enqueued since then
    long long gate_off_until = 0;      // n_flushes at which a gate that was dropped for timing out is tried again (0 = in use)
    bool gate_said = false;
    int no_side_stream = 0;

    int force_generic = 0;
    int fast_exp = 0;
    int no_d64 = 0;
    int no_tap_pair = 0;
    int tap_walk = 0;                 // DAAM_TAP_WALK=1: a binned context's eight-wave head_dim-64 launches walk each layer's windows in one
                                      // workgroup chain (tap_walk_kernel, daam_tap_walk.hip) instead of one chain per window
    int slab_tail_pct = 25;           // DAAM_SLAB_TAIL: percent of a head_dim-40 layer's pixels the slab kernel takes in 16-pixel tiles at the end of the launch
                                      // (SD-v1.5, alternating on one box: 0 -> 2390, 25 -> 2415, 50 -> 2316, 100 -> 2204 maps/s: half-size units cost K traffic)
    int tap_slab = 1;                 // tap_slab_kernel (daam_tap_slab.hip): deferred fp16 layers of head_dim 40 / 80 / 160 in 640-byte slabs of adjacent heads
                                      // (whole 128-byte lines of Q: SD-v1.x); DAAM_TAP_SLAB=0 leaves them to the kernels below
    int tap_chunked = 2;              // tap_chunk_kernel (fp16 layers of any head_dim, one kind of workgroup): 2 = for deferred launches that
                                      // mix head dims (default), 1 = for every fp16 layer (DAAM_TAP_CHUNKED=1), 0 = never (DAAM_TAP_CHUNKED=0)
};

// Entry points may be called with another device current (a pipeline on cuda:1 while the process default is
// cuda:0): streams, events and launches must go to the context's device.  Restores the caller's device on exit.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const DaamCtx* c) {
        if (c && hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

inline size_t acc_elem(int dtype) { return dtype == DAAM_F32 ? 4 : 2; }
inline const char* dtype_name(int dt) { return dt == DAAM_F32 ? "f32" : dt == DAAM_BF16 ? "bf16" : "f16"; }

inline int ensure_zeroed(Layer& l, hipStream_t s)
{
    if (l.zero_pending) {
        HIP_TRY(hipMemsetAsync(l.acc, 0, l.bytes, s));
        l.zero_pending = false;
    }
    return 0;
}

// auxiliary non-blocking streams + fork / join events of a context (multi-kernel tap flushes, multi-class finalize)
hipError_t ensure_aux(DaamCtx* c);

// the table pair of a layer's (h, w) for finalize_rect_kernel, built and uploaded on first use (daam_api.hip): sets l.rtab
int rect_tab(DaamCtx* c, Layer& l);

// a tap call against its layer and the context (daam_tap_api.hip; daam_attend's fused tap asks the same)
int check_qk(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d);
// which running-sum dtypes a pipeline dtype may feed: its own (the reference's behaviour) or f32
inline bool dtypes_compatible(int in_dtype, int acc_dtype) { return acc_dtype == DAAM_F32 || acc_dtype == in_dtype; }

