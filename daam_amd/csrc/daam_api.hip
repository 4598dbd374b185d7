// Host side of libdaam_hip.so: the C ABI declared in include/daam_hip.h.
// Owns no activations; owns (optionally) the running sums, the bicubic tap tables and a
// small pinned upload ring for the per-launch device tables.
#include "daam_ctx.h"
#include "daam_tap_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// which running-sum dtypes a pipeline dtype may feed: its own (the reference's behaviour) or f32
static bool dtypes_compatible(int in_dtype, int acc_dtype) { return acc_dtype == DAAM_F32 || acc_dtype == in_dtype; }

// torch upsample_bicubic2d, align_corners=False, antialias=False:
// scale = in / out in f32; src = scale * (dst + 0.5) - 0.5 (NOT clamped for cubic);
// taps floor(src)-1 .. +2 clamped to the border; A = -0.75.
static void bicubic_table(int in_size, int out_size, int16_t* idx, float* w)
{
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float scale = (float)in_size / (float)out_size;
    for (int j = 0; j < out_size; ++j) {
        const float src = scale * ((float)j + 0.5f) - 0.5f;
        const float f = std::floor(src);
        const float t = src - f;
        const float x0 = t + 1.0f, u = 1.0f - t, x3 = u + 1.0f;
        w[j * 4 + 0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
        w[j * 4 + 1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
        w[j * 4 + 2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
        w[j * 4 + 3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
        for (int a = 0; a < 4; ++a) {
            int v = (int)f - 1 + a;
            v = v < 0 ? 0 : (v > in_size - 1 ? in_size - 1 : v);
            idx[j * 4 + a] = (int16_t)v;
        }
    }
}

// MFMA operand pieces of finalize_up32_mfma_kernel (32 -> 64, fp16-exact banded tap matrix W[o][src]),
// one 16-byte piece per (nt, lane, k): lane = (n = lane & 31, g = lane >> 5)
//   k = 0, 1      : Wx, B of pass 1:  W[32nt + n][16ks + 8g + e],                      ks = k
//   k = 2 + 2t+ks : Wy, A of pass 2:  W[32t + n][16ks + 8(i >> 2) + 4g + (i & 3)]     (contraction index
//                   permuted to the C/D register order of pass 1, see the kernel)
// wx_bf16 (bf16 planes on the pipelined kernel, pass 1 on the bf16 MFMA): 7 pieces per (nt, lane) -- k = 0, 1 hold W' as bf16 bit patterns and
//   k = 6         : E, B of the third pass-1 MFMA:  E[32nt + n][g == 0 ? e : 24 + e]    with W = W' + E, both bf16 numbers
// (W' = W truncated to eight significant bits; the 32 -> 64 table has one entry per border that needs nine: 283/256 = 282/256 + 1/256).
// *ok = 0 when E is not a bf16 number somewhere or has an entry outside source columns 0..7 / 24..31.
static std::vector<_Float16> build_up32_ops(const int16_t* idx, const float* w, bool wx_bf16 = false, int* ok = nullptr)
{
    auto W = [&](int o, int src) {
        float v = 0.f;
        for (int a = 0; a < 4; ++a)
            if (idx[o * 4 + a] == src) v += w[o * 4 + a];
        return (_Float16)v;
    };
    auto trunc_bf16 = [](float v) {
        uint32_t u;
        memcpy(&u, &v, 4);
        u &= 0xffff0000u;
        memcpy(&v, &u, 4);
        return v;
    };
    auto put_bf16 = [](_Float16* dst, float v) {
        const uint16_t bits = f32_to_bf16(v).bits;
        memcpy(dst, &bits, 2);
    };
    const int pieces = wx_bf16 ? 7 : 6;
    if (ok) *ok = 1;
    std::vector<_Float16> ops((size_t)2 * 64 * pieces * 8);
    for (int nt = 0; nt < 2; ++nt)
        for (int lane = 0; lane < 64; ++lane) {
            const int n = lane & 31, g = lane >> 5;
            _Float16* dst = ops.data() + ((size_t)(nt * 64 + lane) * pieces) * 8;
            for (int ks = 0; ks < 2; ++ks)
                for (int e = 0; e < 8; ++e) {
                    const int src = 16 * ks + 8 * g + e;
                    const float v = (float)W(32 * nt + n, src);
                    if (!wx_bf16) { dst[ks * 8 + e] = (_Float16)v; continue; }
                    const float hi = trunc_bf16(v), lo = v - hi;
                    put_bf16(&dst[ks * 8 + e], hi);
                    if (lo != 0.f && ok && (bf16_to_f32(f32_to_bf16(lo)) != lo || (src >= 8 && src < 24))) *ok = 0;
                }
            for (int t = 0; t < 2; ++t)
                for (int ks = 0; ks < 2; ++ks)
                    for (int i = 0; i < 8; ++i)
                        dst[(2 + 2 * t + ks) * 8 + i] = W(32 * t + n, 16 * ks + 8 * (i >> 2) + 4 * g + (i & 3));
            if (wx_bf16)
                for (int e = 0; e < 8; ++e) {
                    const float v = (float)W(32 * nt + n, g == 0 ? e : 24 + e);
                    put_bf16(&dst[6 * 8 + e], v - trunc_bf16(v));
                }
        }
    return ops;
}

// auxiliary non-blocking streams + fork / join events of a context (multi-kernel tap flushes, multi-class finalize)
hipError_t ensure_aux(DaamCtx* c)
{
    if (c->aux_fork) return hipSuccess;
    hipError_t ae = hipEventCreateWithFlags(&c->aux_fork, hipEventDisableTiming);
    for (int i = 0; i < DaamCtx::kAux && ae == hipSuccess; ++i) {
        ae = hipStreamCreateWithFlags(&c->aux_stream[i], hipStreamNonBlocking);
        if (ae == hipSuccess) ae = hipEventCreateWithFlags(&c->aux_join[i], hipEventDisableTiming);
    }
    if (ae == hipSuccess && !c->d_started) {
        ae = hipMalloc(reinterpret_cast<void**>(&c->d_started), sizeof(unsigned));
        if (ae == hipSuccess) ae = hipMemset(c->d_started, 0, sizeof(unsigned));
        c->started_target = 0;
    }
    if (ae == hipSuccess && !c->gate_timeouts) {
        // best effort: without the word the gate still works, its timeouts just go unnoticed
        if (hipHostMalloc(reinterpret_cast<void**>(&c->gate_timeouts), sizeof(unsigned), hipHostMallocMapped) == hipSuccess) {
            *c->gate_timeouts = 0;
            if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->gate_timeouts_dev), c->gate_timeouts, 0) != hipSuccess)
                c->gate_timeouts_dev = nullptr;
        } else {
            c->gate_timeouts = nullptr;
        }
    }
    return ae;
}

static const char* tap_kernel_name(int kd)
{
    return (kd == 65 || kd == 66) ? "tap_d64_kernel" : (kd == 67 || kd == 69) ? "tap_wide_kernel" : kd == 70 ? "tap_chunk_kernel"
           : kd == 71 ? "tap_slab_kernel" : kd == 72 ? "tap_pair_kernel" : kd == 73 ? "tap_walk_kernel" : kd ? "tap_mfma_kernel" : "tap_generic_kernel";
}

extern "C" {

int daam_abi_version(void) { return DAAM_ABI_VERSION; }
const char* daam_last_error(void) { return g_err.c_str(); }

int daam_ctx_create(int max_layers, int tokens, int out_side, int acc_dtype, DaamCtx** out)
{
    if (!out) return fail(DAAM_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_layers <= 0 || max_layers > 4096) return fail(DAAM_E_INVALID, "max_layers %d out of range", max_layers);
    if (tokens <= 0 || tokens > kMaxTokens) return fail(DAAM_E_INVALID, "tokens %d not in 1..%d", tokens, kMaxTokens);
    if (out_side <= 0 || out_side > 128) return fail(DAAM_E_INVALID, "out_side %d not in 1..128", out_side);
    if (acc_dtype != DAAM_F16 && acc_dtype != DAAM_F32 && acc_dtype != DAAM_BF16) return fail(DAAM_E_INVALID, "acc_dtype %d", acc_dtype);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail((int)hipErrorNoDevice, "no HIP device");
    DaamCtx* c = new DaamCtx();
    HIP_TRY(hipGetDevice(&c->device));
    c->max_layers = max_layers;
    c->tokens = tokens;
    c->out_side = out_side;
    c->acc_dtype = acc_dtype;
    c->layers.resize(max_layers);
    c->tap_steps.assign(max_layers, 0);
    hipError_t e = c->ring.init();
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_tab_idx), sizeof(int16_t) * kMaxTabs * out_side * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_tab_w), sizeof(float) * kMaxTabs * out_side * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_fin_tab), DaamCtx::kFinTabCap);
    if (e != hipSuccess) {
        daam_ctx_destroy(c);
        return fail((int)e, "context allocation: %s", hipGetErrorString(e));
    }
    const char* fg = getenv("DAAM_FORCE_GENERIC");
    c->force_generic = fg && fg[0] == '1';
    const char* nm = getenv("DAAM_NO_MFMA_FINALIZE");
    c->no_mfma_finalize = nm && nm[0] == '1';
    const char* nfs = getenv("DAAM_NO_FOLD_SAME");
    c->no_fold_same = nfs && nfs[0] == '1';
    const char* nsg = getenv("DAAM_NO_START_GATE");
    c->no_start_gate = nsg && nsg[0] == '1';
    const char* npp = getenv("DAAM_NO_PIPE_FINALIZE");
    c->no_pipe_finalize = npp && npp[0] == '1';
    const char* npf = getenv("DAAM_NO_PAIRED_FINALIZE");
    c->no_paired_finalize = npf && npf[0] == '1';
    const char* w8 = getenv("DAAM_TAP_W8");
    c->no_w8 = w8 && w8[0] == '0';
    const char* tsy = getenv("DAAM_TAP_SYNC");              // 0: the head_dim-64 tap's step protocol before the counted waits
    c->tap_sync = !(tsy && tsy[0] == '0');
    const char* nfc = getenv("DAAM_NO_FIN_CACHE");
    c->no_fin_cache = nfc && nfc[0] == '1';
    const char* n16 = getenv("DAAM_NO_D64");            // debugging: 32x32-tile kernel also for head_dim 64
    c->no_d64 = n16 && n16[0] == '1';
    const char* nss = getenv("DAAM_NO_SIDE_STREAM");        // debugging / A-B: every tap kernel of a flush on the caller's stream
    c->no_side_stream = nss && nss[0] == '1';
    const char* stl = getenv("DAAM_SLAB_TAIL");
    if (stl && stl[0]) c->slab_tail_pct = std::max(0, std::min(100, atoi(stl)));
    const char* tsl = getenv("DAAM_TAP_SLAB");
    c->tap_slab = !(tsl && tsl[0] == '0');
    const char* tck = getenv("DAAM_TAP_CHUNKED");           // daam_tap_chunk.hip: unset = launches that mix head dims, 1 = always, 0 = never
    c->tap_chunked = !tck || !tck[0] ? 2 : tck[0] == '1' ? 1 : tck[0] == '0' ? 0 : 2;
    const char* ntp = getenv("DAAM_TAP_PAIR");              // 1: chains that share Q pair up on tap_pair_kernel; default: separate chains
    c->no_tap_pair = !(ntp && ntp[0] == '1');
    const char* twk = getenv("DAAM_TAP_WALK");              // 1: a layer's time windows walk through one workgroup chain (tap_walk_kernel)
    c->tap_walk = twk && twk[0] == '1';

    // softmax flavour of the MFMA tap: fast (default; exponent by one mixed-precision FMA, ~1e-6 relative,
    // same deviation class as the f32 summation order of q.k -- DESIGN.md section 3.1) or compensated
    // (DAAM_STRICT_EXP=1: ~1 ulp f32 like the reference's expf)
    const char* se = getenv("DAAM_STRICT_EXP");
    c->fast_exp = !(se && se[0] == '1');
    *out = c;
    return 0;
}

int daam_ctx_destroy(DaamCtx* c)
{
    if (!c) return 0;
    DeviceGuard on_device(c);
    (void)hipDeviceSynchronize();
    c->ring.destroy();
    for (auto& l : c->layers)
        if (l.owned && l.acc) (void)hipFree(l.acc);
    for (auto& pair : c->prof_ev)
        for (auto& ev : pair)
            if (ev) (void)hipEventDestroy(ev);
    for (auto& pair : c->hist_ev)
        for (auto& ring : pair)
            for (auto ev : ring)
                if (ev) (void)hipEventDestroy(ev);
    if (c->aux_fork) (void)hipEventDestroy(c->aux_fork);
    if (c->d_started) (void)hipFree(c->d_started);
    if (c->gate_timeouts) (void)hipHostFree(c->gate_timeouts);
    for (auto& ev : c->aux_join)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& st : c->aux_stream)
        if (st) (void)hipStreamDestroy(st);
    if (c->clk_stream) (void)hipStreamDestroy(c->clk_stream);
    if (c->clk_host) (void)hipHostFree(c->clk_host);
    if (c->d_up32_ops) (void)hipFree(c->d_up32_ops);
    if (c->d_up32_ops_bf16) (void)hipFree(c->d_up32_ops_bf16);
    if (c->d_zero_planes) (void)hipFree(c->d_zero_planes);
    if (c->d_fin_tab) (void)hipFree(c->d_fin_tab);
    if (c->d_tab_idx) (void)hipFree(c->d_tab_idx);
    if (c->d_tab_w) (void)hipFree(c->d_tab_w);
    if (c->bin_scratch) (void)hipFree(c->bin_scratch);
    delete c;
    return 0;
}

int daam_layer_configure(DaamCtx* c, int layer, int heads, int side, int factor, void* acc)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    if (layer < 0 || layer >= c->max_layers) return fail(DAAM_E_INVALID, "layer %d out of range", layer);
    if (heads <= 0 || side <= 0 || side > 1024) return fail(DAAM_E_INVALID, "heads %d / side %d", heads, side);
    DeviceGuard on_device(c);
    for (auto& p : c->pending)
        if (p.layer % c->max_layers == layer) return fail(DAAM_E_STATE, "layer %d re-configured with un-flushed taps pending", layer);
    Layer& l = c->layers[layer];
    if (l.owned && l.acc) { HIP_TRY(hipFree(l.acc)); }
    l = Layer();
    l.heads = heads;
    l.side = side;
    l.hw = side * side;
    l.factor = factor;
    l.bytes = (size_t)heads * c->tokens * l.hw * acc_elem(c->acc_dtype);
    const int nb = std::max(1, c->n_bins);                     // a binned layer's buffer holds every window
    if (acc) {
        l.acc = acc;
    } else {
        HIP_TRY(hipMalloc(&l.acc, l.bytes * nb));
        HIP_TRY(hipMemset(l.acc, 0, l.bytes * nb));
        l.owned = true;
    }
    if (side != c->out_side) {
        int tab = -1;
        for (size_t i = 0; i < c->tab_sides.size(); ++i)
            if (c->tab_sides[i] == side) tab = (int)i;
        if (tab < 0) {
            if ((int)c->tab_sides.size() >= kMaxTabs) return fail(DAAM_E_UNSUPPORTED, "more than %d distinct map sizes", kMaxTabs);
            tab = (int)c->tab_sides.size();
            std::vector<int16_t> idx(c->out_side * 4);
            std::vector<float> w(c->out_side * 4);
            bicubic_table(side, c->out_side, idx.data(), w.data());
            HIP_TRY(hipMemcpy(c->d_tab_idx + (size_t)tab * c->out_side * 4, idx.data(), idx.size() * sizeof(int16_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(c->d_tab_w + (size_t)tab * c->out_side * 4, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
            c->tab_sides.push_back(side);
            // can the banded tap matrix be an fp16 MFMA operand without rounding?
            int exact = 1;
            for (int j = 0; j < c->out_side && exact; ++j)
                for (int a = 0; a < 4 && exact; ++a) {
                    float merged = 0.f;                    // taps clamped onto the same border column add up
                    for (int b2 = 0; b2 < 4; ++b2)
                        if (idx[j * 4 + b2] == idx[j * 4 + a]) merged += w[j * 4 + b2];
                    exact = ((float)(_Float16)merged == merged) && ((float)(_Float16)w[j * 4 + a] == w[j * 4 + a]);
                }
            c->tab_fp16_exact.push_back(exact);
            if (exact && side == 32 && c->out_side == 64 && !c->d_up32_ops) {
                std::vector<_Float16> ops = build_up32_ops(idx.data(), w.data());
                HIP_TRY(hipMalloc(&c->d_up32_ops, ops.size() * sizeof(_Float16)));
                HIP_TRY(hipMemcpy(c->d_up32_ops, ops.data(), ops.size() * sizeof(_Float16), hipMemcpyHostToDevice));
                // bf16 planes: W = W' + E as two bf16 operands (build_up32_ops checks that the table splits that way)
                int bf_ok = 0;
                ops = build_up32_ops(idx.data(), w.data(), true, &bf_ok);
                if (bf_ok) {
                    HIP_TRY(hipMalloc(&c->d_up32_ops_bf16, ops.size() * sizeof(_Float16)));
                    HIP_TRY(hipMemcpy(c->d_up32_ops_bf16, ops.data(), ops.size() * sizeof(_Float16), hipMemcpyHostToDevice));
                }
                c->up32_tab = tab;
                const size_t zb = (size_t)c->tokens * 32 * 32 * sizeof(float);
                HIP_TRY(hipMalloc(&c->d_zero_planes, zb));
                HIP_TRY(hipMemset(c->d_zero_planes, 0, zb));
            }
        }
        l.tab = tab;
    }
    l.configured = true;
    for (int b = 1; b < nb; ++b) {                             // window b: its slice of the same buffer
        Layer& w = c->layers[(size_t)b * c->max_layers + layer];
        w = l;
        w.acc = static_cast<char*>(l.acc) + (size_t)b * l.bytes;
        w.owned = false;
    }
    return 0;
}

int daam_layer_acc(DaamCtx* c, int layer, void** acc, size_t* bytes)
{
    if (!c || layer < 0 || layer >= c->max_layers || !c->layers[layer].configured)
        return fail(DAAM_E_STATE, "layer %d not configured", layer);
    if (acc) *acc = c->layers[layer].acc;
    if (bytes) *bytes = c->layers[layer].bytes * std::max(1, c->n_bins);
    return 0;
}

int daam_ctx_set_time_bins(DaamCtx* c, int n_bins, const int32_t* first_step)
{
    if (!c || !first_step) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_bins < 1 || n_bins > kMaxBins) return fail(DAAM_E_INVALID, "n_bins %d not in 1..%d", n_bins, kMaxBins);
    if (first_step[0] != 0) return fail(DAAM_E_INVALID, "the first window starts at step %d, not 0", first_step[0]);
    for (int b = 1; b < n_bins; ++b)
        if (first_step[b] <= first_step[b - 1])
            return fail(DAAM_E_INVALID, "window starts not strictly increasing: %d after %d", first_step[b], first_step[b - 1]);
    for (const Layer& l : c->layers)
        if (l.configured) return fail(DAAM_E_STATE, "time windows must be set before any layer is configured");
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "time windows set with deferred taps pending");
    c->n_bins = n_bins;
    for (int b = 0; b < kMaxBins; ++b) c->bin_first[b] = b < n_bins ? first_step[b] : 0;
    c->layers.assign((size_t)n_bins * c->max_layers, Layer());
    std::fill(c->tap_steps.begin(), c->tap_steps.end(), 0);
    return 0;
}

int daam_tap_steps(DaamCtx* c, int layer, int* steps)
{
    if (!c || !steps) return fail(DAAM_E_INVALID, "NULL argument");
    if (layer < 0 || layer >= c->max_layers) return fail(DAAM_E_INVALID, "layer %d out of range", layer);
    *steps = c->tap_steps[layer];
    return 0;
}

int daam_layer_touch(DaamCtx* c, int layer, void* stream)
{
    if (!c || layer < 0 || layer >= c->max_layers || !c->layers[layer].configured)
        return fail(DAAM_E_STATE, "layer %d not configured", layer);
    if (c->n_bins) return fail(DAAM_E_UNSUPPORTED, "a time-binned context does not take hand-written sums (which window?)");
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "layer touched with deferred taps pending: flush first");
    DeviceGuard on_device(c);
    Layer& l = c->layers[layer];
    int zrc = ensure_zeroed(l, (hipStream_t)stream);       // a reset still owed to the buffer happens first, on this stream
    if (zrc) return zrc;
    l.dirty = true;                                        // later taps add to the sums, the next reset clears them
    return 0;
}

int daam_layer_release(DaamCtx* c, int layer)
{
    if (!c || layer < 0 || layer >= c->max_layers) return fail(DAAM_E_INVALID, "layer %d out of range", layer);
    for (auto& p : c->pending)
        if (p.layer % c->max_layers == layer) return fail(DAAM_E_STATE, "layer %d released with un-flushed taps pending", layer);
    Layer& l = c->layers[layer];
    if (l.owned && l.acc) {
        DeviceGuard on_device(c);
        HIP_TRY(hipFree(l.acc));
    }
    l = Layer();                                               // unconfigured: no later call touches the old buffer
    for (int b = 1; b < c->n_bins; ++b) c->layers[(size_t)b * c->max_layers + layer] = Layer();
    return 0;
}

int daam_reset(DaamCtx* c, void* stream)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    c->drop_pending();
    c->prep_out = c->fold_out = nullptr;
    std::fill(c->tap_steps.begin(), c->tap_steps.end(), 0);    // step indices of the time windows restart
    (void)stream;
    for (auto& l : c->layers)
        if (l.configured) {
            // lazy: a layer that is tapped again is overwritten by its first launch (TapLayer.fresh),
            // so the 221 MB of memsets per generation are only paid for paths that read the sums first
            l.zero_pending = l.zero_pending || l.dirty;
            l.dirty = false;
        }
    return 0;
}

static int check_qk(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d)
{
    if (!c || !d || !q || !k) return fail(DAAM_E_INVALID, "NULL argument");
    if (layer < 0 || layer >= c->max_layers || !c->layers[layer].configured)
        return fail(DAAM_E_STATE, "layer %d not configured", layer);
    const Layer& l = c->layers[layer];
    if (d->in_dtype != DAAM_F16 && d->in_dtype != DAAM_F32 && d->in_dtype != DAAM_BF16) return fail(DAAM_E_INVALID, "in_dtype %d", d->in_dtype);
    if (!dtypes_compatible(d->in_dtype, c->acc_dtype))
        return fail(DAAM_E_INVALID, "activations of dtype %d cannot feed running sums of dtype %d (own dtype or f32)", d->in_dtype, c->acc_dtype);
    if (d->tokens != c->tokens) return fail(DAAM_E_INVALID, "tokens %d != context size %d (reference gate, trace.py:289)", d->tokens, c->tokens);
    if (d->batch <= 0 || d->heads <= 0 || d->head_dim <= 0 || d->head_dim > 1024)
        return fail(DAAM_E_INVALID, "batch %d heads %d head_dim %d", d->batch, d->heads, d->head_dim);
    const int bh = d->batch * d->heads;
    if (bh - bh / 2 != l.heads) return fail(DAAM_E_INVALID, "layer %d holds %d heads, call keeps %d", layer, l.heads, bh - bh / 2);
    if (d->hw != l.hw) return fail(DAAM_E_INVALID, "layer %d holds %d positions, call has %d", layer, l.hw, d->hw);
    return 0;
}

static void fill_layer(const DaamCtx* c, const Layer& l, const DaamQKDesc& d, int tile_pixels, TapLayer* t)
{
    const int bh = d.batch * d.heads;
    t->acc = l.acc;
    t->heads_kept = l.heads;
    t->bh_first = bh / 2;
    t->heads = d.heads;
    t->hw = d.hw;
    t->head_dim = d.head_dim;
    t->tiles_per_head = (d.hw + tile_pixels - 1) / tile_pixels;
    t->wg_begin = 0;
    t->n_steps = 1;
    t->ptr_begin = 0;
    t->round_logits = d.round_logits;
    t->scale = d.scale;
    t->fresh = l.dirty ? 0 : 1;
    t->px_begin = 0;
    t->px_end = d.hw;
    t->tile_px = tile_pixels;
    t->q_sb = d.q_stride_b; t->q_sh = d.q_stride_h; t->q_sp = d.q_stride_p;
    t->k_sb = d.k_stride_b; t->k_sh = d.k_stride_h; t->k_st = d.k_stride_t;
    (void)c;
}

static bool use_d64_bf16(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k);
static bool use_chunk(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k);

static bool use_mfma(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (c->force_generic) return false;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return false;
    if (d.in_dtype == DAAM_BF16) return use_d64_bf16(c, d, q, k) || use_chunk(c, d, q, k);
    return tap_mfma_supported(d.in_dtype, d.head_dim, d.tokens, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b,
                              d.q_stride_h, d.k_stride_b, d.k_stride_h);
}

// kernel choice for an MFMA-capable call: 65 = 16x16-tile head_dim-64 kernel (default for d = 64),
// else the k-step count of the generic 32x32-tile MFMA kernel
static int mfma_kind(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k);

// The specialised tap kernels address Q and K with 32-bit BYTE offsets from the tensor pointers: every element a call can
// address -- (batch - 1) * stride_b + (heads - 1) * stride_h + (rows - 1) * row stride + head_dim -- must stay below 2^30 elements
// (views into a large fused buffer with unusual strides fall back to the any-shape kernel instead of wrapping).
static bool offsets_fit_32(const DaamQKDesc& d)
{
    const int64_t lim = (int64_t)1 << 30;
    const int64_t s[] = {d.q_stride_b, d.q_stride_h, d.q_stride_p, d.k_stride_b, d.k_stride_h, d.k_stride_t};
    for (int64_t v : s)
        if (v < 0 || v >= lim) return false;
    const int64_t q_max = (int64_t)(d.batch - 1) * d.q_stride_b + (int64_t)(d.heads - 1) * d.q_stride_h + (int64_t)(d.hw - 1) * d.q_stride_p + d.head_dim;
    const int64_t k_max = (int64_t)(d.batch - 1) * d.k_stride_b + (int64_t)(d.heads - 1) * d.k_stride_h + (int64_t)(d.tokens - 1) * d.k_stride_t + d.head_dim;
    return q_max < lim && k_max < lim;
}

static bool use_d64(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return !c->no_d64 && offsets_fit_32(d) && tap_d64_supported(d.head_dim, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h,
                                           d.k_stride_b, d.k_stride_h, q, k);
}

// bf16 pipelines: only the 16x16-tile kernel has a bf16 variant (head_dim <= 64, 77 tokens, bf16-rounded logits);
// everything else of a bf16 pipeline runs on the any-shape kernel
static bool use_d64_bf16(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return d.in_dtype == DAAM_BF16 && !c->no_d64 && c->fast_exp && d.round_logits && d.tokens == 77 && d.hw % 8 == 0 && offsets_fit_32(d) &&
           tap_d64_supported(d.head_dim, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h, d.k_stride_b,
                             d.k_stride_h, q, k);
}

// 64 < head_dim <= 160 on fp16 pipelines (SD-v1.5's 80 / 160): the 16x16-tile kernel with 3 or 5 k-steps (daam_tap_wide.hip)
static bool use_wide(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return !c->no_d64 && (c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32) && offsets_fit_32(d) &&
           (int64_t)d.batch * d.q_stride_b < ((int64_t)1 << 30) &&
           tap_wide_supported(d.in_dtype, d.head_dim, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h, d.k_stride_b,
                              d.k_stride_h, q, k);
}

// the chunked kernel (daam_tap_chunk.hip) can take this call: fp16 layers of any head_dim (multiple of 8, <= 256), and bf16 layers (bf16
// or f32 sums, bf16-rounded logits, the fast softmax -- what the bf16 head_dim-64 kernel asks for; validated on the chip in round 4)
static bool chunk_ok(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (!c->tap_chunked || c->no_d64 || c->force_generic || d.tokens != 77 || !offsets_fit_32(d)) return false;
    if (d.in_dtype == DAAM_BF16) {
        if (!c->fast_exp || !d.round_logits || !(c->acc_dtype == DAAM_BF16 || c->acc_dtype == DAAM_F32)) return false;
    } else if (!(c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32)) {
        return false;
    }
    return tap_chunk_supported(d.in_dtype, d.head_dim, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h, d.k_stride_b,
                               d.k_stride_h, (int64_t)d.batch * d.q_stride_b, q, k);
}

// the slab kernel (daam_tap_slab.hip) can take this deferred call: fp16 Q / K, fp16 or f32 sums, head_dim 40 / 80 / 160 with the heads
// adjacent in the rows
static bool slab_ok(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (!c->tap_slab || c->no_d64 || c->force_generic || d.tokens != 77 || d.in_dtype != DAAM_F16 || !offsets_fit_32(d)) return false;
    if (!(c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32)) return false;
    return tap_slab_supported(d.in_dtype, d.batch, d.heads, d.head_dim, d.hw, d.q_stride_p, d.k_stride_t, d.q_stride_b, d.q_stride_h, d.k_stride_b,
                              d.k_stride_h, (int64_t)d.batch * d.q_stride_b, q, k);
}

// DAAM_TAP_CHUNKED=1: every such call.  Default (2): the deferred launches that mix head dims (daam_tap_flush), and bf16 layers with
// head_dim > 64 -- no other MFMA kernel has a bf16 form for them (the any-shape kernel is ~45x slower per step).
static bool use_chunk(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (c->tap_chunked == 1) return chunk_ok(c, d, q, k);
    return c->tap_chunked == 2 && d.in_dtype == DAAM_BF16 && d.head_dim > 64 && chunk_ok(c, d, q, k);
}

static int mfma_kind(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (use_chunk(c, d, q, k)) return 70;
    if (d.in_dtype == DAAM_BF16) return 66;                   // only reached when use_d64_bf16() holds
    if (use_d64(c, d, q, k)) return 65;
    if (use_wide(c, d, q, k)) return d.head_dim <= 96 ? 67 : 69;
    return tap_mfma_ksteps(d.head_dim);
}

int daam_tap_qk(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d, void* stream)
{
    int rc = check_qk(c, layer, q, k, d);
    if (rc) return rc;
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "immediate tap with deferred taps pending: flush first");
    DeviceGuard on_device(c);
    const int slot = c->slot_of(layer);                        // the window of this step (= layer without windows)
    const bool mfma = use_mfma(c, *d, q, k);
    if (!mfma && (rc = ensure_zeroed(c->layers[slot], (hipStream_t)stream))) return rc;
    TapLaunch L;
    memset(&L, 0, sizeof L);
    fill_layer(c, c->layers[slot], *d, mfma ? tap_mfma_tile_pixels() : kTapPixels, &L.one);
    L.one_ptr.q = q;
    L.one_ptr.k = k;
    L.n_layers = 1;
    L.tokens = c->tokens;
    L.total_wgs = L.one.heads_kept * L.one.tiles_per_head;
    L.wgs_per_xcd = (L.total_wgs + 7) / 8;
    c->last_block[0] = 256;
    const int kd1 = mfma ? mfma_kind(c, *d, q, k) : 0;
    hipError_t e = (kd1 == 65 || kd1 == 66) ? launch_tap_d64(L, d->in_dtype, c->acc_dtype, c->fast_exp && d->round_logits, d->head_dim == 64, 0, c->tap_sync, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0])
                   : (kd1 == 67 || kd1 == 69) ? launch_tap_wide(L, c->acc_dtype, d->head_dim, c->fast_exp && d->round_logits, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0])
                   : kd1 == 70 ? launch_tap_chunk(L, d->in_dtype, c->acc_dtype, c->fast_exp && d->round_logits, 0, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0])
                   : mfma ? launch_tap_mfma(L, c->acc_dtype, d->head_dim, c->fast_exp && d->round_logits, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0])
                        : launch_tap_generic(L, d->in_dtype, c->acc_dtype, d->head_dim, (hipStream_t)stream,
                                             &c->last_grid[0], &c->last_lds[0]);
    if (e != hipSuccess) return fail((int)e, "tap launch: %s", hipGetErrorString(e));
    c->last_kernels[0] = tap_kernel_name(kd1);
    c->layers[slot].dirty = true;
    c->layers[slot].zero_pending = false;
    ++c->tap_steps[layer];
    return 0;
}

int daam_attend_supported(const DaamAttendDesc* d, const void* q, const void* k, const void* v, const void* out)
{
    if (!d || !q || !k || !v || !out) return 0;
    const int64_t strides[] = {d->qk.q_stride_b, d->qk.q_stride_h, d->qk.q_stride_p, d->qk.k_stride_b, d->qk.k_stride_h,
                               d->qk.k_stride_t, d->v_stride_b, d->v_stride_h, d->v_stride_t, d->o_stride_b, d->o_stride_h,
                               d->o_stride_p};
    const void* ptrs[] = {q, k, v, out};
    // hw % 8: the fused tap updates the running sums in 16-byte row pieces (8 fp16 pixels), rows must start aligned
    if (d->qk.batch <= 0 || d->qk.heads <= 0 || d->qk.hw <= 0 || d->qk.hw % 8 != 0) return 0;
    return attend_d64_supported(d->qk.in_dtype, d->qk.head_dim, d->qk.tokens, strides, 12, ptrs, 4) ? 1 : 0;
}

int daam_attend(DaamCtx* c, int layer, const void* q, const void* k, const void* v, void* out, const DaamAttendDesc* d,
                int tap, void* stream)
{
    if (!c || !d || !q || !k || !v || !out) return fail(DAAM_E_INVALID, "NULL argument");
    if (!daam_attend_supported(d, q, k, v, out))
        return fail(DAAM_E_UNSUPPORTED, "daam_attend: fp16 / bf16, head_dim %% 8 == 0 up to 160, 77 tokens, hw %% 8 == 0, strides %% 8 == 0, 16-byte aligned pointers only");
    if (d->qk.in_dtype == DAAM_BF16 && !d->qk.round_logits)
        return fail(DAAM_E_UNSUPPORTED, "daam_attend: bf16 pipelines with upcast_attention (f32 logits) take the framework's attention");
    if (!dtypes_compatible(d->qk.in_dtype, c->acc_dtype))
        return fail(DAAM_E_UNSUPPORTED, "daam_attend: activations of dtype %d on a context whose sums are dtype %d", d->qk.in_dtype, c->acc_dtype);
    if (d->qk.tokens != c->tokens) return fail(DAAM_E_INVALID, "tokens %d != context size %d", d->qk.tokens, c->tokens);
    if (tap) {
        int rc = check_qk(c, layer, q, k, &d->qk);
        if (rc) return rc;
        if (!c->pending.empty()) return fail(DAAM_E_STATE, "fused tap with deferred taps pending: flush first");
    }
    DeviceGuard on_device(c);
    const int slot = tap ? c->slot_of(layer) : layer;
    AttendLaunch L;
    memset(&L, 0, sizeof L);
    L.q = q; L.k = k; L.v = v; L.out = out;
    L.batch = d->qk.batch; L.heads = d->qk.heads; L.hw = d->qk.hw; L.head_dim = d->qk.head_dim;
    L.tiles_per_head = (d->qk.hw + tap_mfma_tile_pixels() - 1) / tap_mfma_tile_pixels();
    L.total_wgs = L.batch * L.heads * L.tiles_per_head;
    L.wgs_per_xcd = (L.total_wgs + 7) / 8;
    L.bh_first = (d->qk.batch * d->qk.heads) / 2;
    L.round_logits = d->qk.round_logits;
    L.scale = d->qk.scale;
    L.q_sb = d->qk.q_stride_b; L.q_sh = d->qk.q_stride_h; L.q_sp = d->qk.q_stride_p;
    L.k_sb = d->qk.k_stride_b; L.k_sh = d->qk.k_stride_h; L.k_st = d->qk.k_stride_t;
    L.v_sb = d->v_stride_b; L.v_sh = d->v_stride_h; L.v_st = d->v_stride_t;
    L.o_sb = d->o_stride_b; L.o_sh = d->o_stride_h; L.o_sp = d->o_stride_p;
    if (tap) {
        L.acc = c->layers[slot].acc;
        L.fresh = c->layers[slot].dirty ? 0 : 1;
    }
    int grid = 0, lds = 0;
    hipError_t e = launch_attend_d64(L, d->qk.in_dtype, c->acc_dtype, c->fast_exp && d->qk.round_logits, (hipStream_t)stream, &grid, &lds);
    if (e != hipSuccess) return fail((int)e, "attend launch: %s", hipGetErrorString(e));
    if (tap) {
        c->last_grid[0] = grid;
        c->last_block[0] = 256;
        c->last_lds[0] = lds;
        c->layers[slot].dirty = true;
        c->layers[slot].zero_pending = false;
        ++c->tap_steps[layer];
    }
    return 0;
}

// record one validated call for `slot` (a layer, or a (window, layer) slot of a binned context)
static int enqueue_slot(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d)
{
    if (!c->pending.empty() && c->pending.front().d.in_dtype != d->in_dtype)
        return fail(DAAM_E_STATE, "mixed activation dtypes in one deferred batch: flush first");
    if (c->pending_count.size() != c->layers.size()) {
        c->pending_count.assign(c->layers.size(), 0);
        c->pending_last.assign(c->layers.size(), -1);
    }
    if (c->pending_count[layer] > 0) {
        // every recorded step of a layer must share shape and strides
        const DaamQKDesc& o = c->pending[c->pending_last[layer]].d;
        if (o.batch != d->batch || o.heads != d->heads || o.head_dim != d->head_dim ||
            o.round_logits != d->round_logits || o.scale != d->scale || o.q_stride_b != d->q_stride_b ||
            o.q_stride_h != d->q_stride_h || o.q_stride_p != d->q_stride_p || o.k_stride_b != d->k_stride_b ||
            o.k_stride_h != d->k_stride_h || o.k_stride_t != d->k_stride_t)
            return fail(DAAM_E_STATE, "layer %d changed shape inside a deferred batch: flush first", layer);
        if (c->pending_count[layer] >= tap_mfma_max_steps())
            return fail(DAAM_E_STATE, "layer %d already has %d un-flushed steps: flush first", layer,
                        c->pending_count[layer]);
    }
    c->pending_last[layer] = (int)c->pending.size();
    ++c->pending_count[layer];
    c->pending.push_back({layer, q, k, *d});
    return 0;
}

int daam_tap_qk_enqueue(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d)
{
    int rc = check_qk(c, layer, q, k, d);
    if (rc) return rc;
    rc = enqueue_slot(c, c->slot_of(layer), q, k, d);
    if (!rc) ++c->tap_steps[layer];
    return rc;
}

int daam_tap_qk_enqueue_many(DaamCtx* c, int n, const int32_t* layers, const void* const* q, const void* const* k,
                             const DaamQKDesc* const* descs)
{
    if (!c || n < 0 || (n > 0 && (!layers || !q || !k || !descs))) return fail(DAAM_E_INVALID, "NULL argument");
    const size_t before = c->pending.size();
    const std::vector<int> steps_before = c->tap_steps;
    for (int i = 0; i < n; ++i) {
        int rc = daam_tap_qk_enqueue(c, layers[i], q[i], k[i], descs[i]);
        if (rc) {
            // all or nothing: rebuild the per-slot bookkeeping for the surviving prefix, and the step counts
            std::vector<Pending> keep(c->pending.begin(), c->pending.begin() + before);
            c->drop_pending();
            c->tap_steps = steps_before;
            for (auto& p : keep) (void)enqueue_slot(c, p.layer, p.q, p.k, &p.d);
            return rc;
        }
    }
    return 0;
}

int daam_tap_pending(DaamCtx* c, int* n_calls, int* max_steps)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    std::vector<int> cnt(c->layers.size(), 0);
    int mx = 0;
    for (auto& p : c->pending) mx = std::max(mx, ++cnt[p.layer]);
    if (n_calls) *n_calls = (int)c->pending.size();
    if (max_steps) *max_steps = mx;
    return 0;
}

int daam_tap_flush(DaamCtx* c, void* stream)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    if (c->pending.empty()) return 0;
    DeviceGuard on_device(c);
    hipStream_t s = (hipStream_t)stream;
    const int in_dtype = c->pending.front().d.in_dtype;
    // group the recorded calls by layer (first-seen order, steps in recorded order), and the
    // layers by kernel: MFMA k-step count ceil(d/16), or 0 = generic kernel.
    std::vector<int> order;
    std::vector<int> slot(c->layers.size(), -1);              // (a binned context: per (window, layer) slot)
    std::vector<std::vector<const Pending*>> per;
    std::vector<int> kind;
    for (auto& p : c->pending) {
        if (slot[p.layer] < 0) {
            slot[p.layer] = (int)order.size();
            order.push_back(p.layer);
            per.emplace_back();
            kind.push_back(tap_mfma_ksteps(p.d.head_dim));
        }
        const int i = slot[p.layer];
        if (!use_mfma(c, p.d, p.q, p.k)) kind[i] = 0;
        else if (kind[i] != 0) {
            // every step of the layer must qualify for the specialised kernel, else the generic MFMA one
            const int want = mfma_kind(c, p.d, p.q, p.k);
            if (per[i].empty()) kind[i] = want;
            else if (kind[i] != want) kind[i] = p.d.in_dtype == DAAM_BF16 ? 0 : tap_mfma_ksteps(p.d.head_dim);
        }
        per[i].push_back(&p);
    }
    // A launch that mixes head dims (SD-v1.5: 40 / 80 / 160 = the head_dim-64 kernel and the two wide ones side by side, whose LDS
    // footprints keep them from sharing CUs): every such layer on the chunked kernel instead -- ONE kind of workgroup, one launch,
    // no side streams, bit-identical sums (tests/test_gpu_chunked.py; +11 ... 13 % heat maps / s on the SD-v1.5 workload).
    if (c->tap_chunked == 2) {
        bool k65 = false, k67 = false, k69 = false;
        for (int kd : kind) {
            k65 = k65 || kd == 65;
            k67 = k67 || kd == 67;
            k69 = k69 || kd == 69;
        }
        bool k66 = false, k70 = false;                         // bf16 pipelines: head_dim <= 64 -> 66, wider heads -> 70 (use_chunk)
        for (int kd : kind) {
            k66 = k66 || kd == 66;
            k70 = k70 || kd == 70;
        }
        if ((int)k65 + (int)k67 + (int)k69 >= 2 || (k66 && k70)) {   // (an SDXL launch -- one kind -- never gets here: no per-call checks)
            bool all_ok = true;
            for (size_t i = 0; i < kind.size() && all_ok; ++i)
                if (kind[i] == 65 || kind[i] == 66 || kind[i] == 67 || kind[i] == 69)
                    for (const Pending* p : per[i]) all_ok = all_ok && chunk_ok(c, p->d, p->q, p->k);
            if (all_ok)
                for (int& kd : kind)
                    if (kd == 65 || kd == 66 || kd == 67 || kd == 69) kd = 70;
        }
    }
    // fp16 layers of head_dim 40 / 80 / 160 (SD-v1.x) whose every recorded step qualifies: the slab kernel -- whole 128-byte lines of Q,
    // ONE launch for the three head dims (bit-identical sums: tests/test_gpu_slab.py).  DAAM_TAP_CHUNKED=0 / 1 pin the older kernels.
    if (c->tap_slab && c->tap_chunked == 2 && in_dtype == DAAM_F16) {
        for (size_t i = 0; i < kind.size(); ++i) {
            if (!(kind[i] == 65 || kind[i] == 67 || kind[i] == 69 || kind[i] == 70) || !tap_slab_heads(per[i][0]->d.head_dim)) continue;
            bool ok = true;
            for (const Pending* p : per[i]) ok = ok && slab_ok(c, p->d, p->q, p->k);
            if (ok) kind[i] = 71;
        }
    }
    // Chains that read the same recorded Q (probes): head_dim-64 fp16 chains with fp16 sums pair up on tap_pair_kernel -- chain A
    // any such chain, chain B one whose K is the same pointer at every step (a probe); in recorded order: generation + probe 0, probe 1 +
    // probe 2, ...  The partner's kind becomes -1 (it rides with its chain A).  Unpaired chains keep their kernel.  Only with DAAM_TAP_PAIR=1:
    // measured slower than separate chains for one and two probes, 4 % faster for four, so separate chains are the default.
    std::vector<int> partner(order.size(), -1);
    if (!c->no_tap_pair && !c->no_w8 && in_dtype == DAAM_F16 && c->acc_dtype == DAAM_F16) {
        auto fixed_k = [&](size_t i) {
            for (const Pending* p : per[i]) if (p->k != per[i][0]->k) return false;
            return true;
        };
        auto same_q = [&](size_t a, size_t b) {
            if (per[a].size() != per[b].size()) return false;
            const DaamQKDesc &x = per[a][0]->d, &y = per[b][0]->d;
            if (x.head_dim != 64 || y.head_dim != 64 || x.hw != y.hw || x.heads != y.heads || x.batch != y.batch ||
                x.q_stride_b != y.q_stride_b || x.q_stride_h != y.q_stride_h || x.q_stride_p != y.q_stride_p ||
                x.k_stride_h != y.k_stride_h || x.k_stride_t != y.k_stride_t || x.scale != y.scale || x.round_logits != y.round_logits ||
                c->layers[order[a]].heads != c->layers[order[b]].heads)
                return false;
            for (size_t st = 0; st < per[a].size(); ++st) if (per[a][st]->q != per[b][st]->q) return false;
            return true;
        };
        for (size_t a = 0; a < order.size(); ++a) {
            if (kind[a] != 65 || partner[a] >= 0) continue;
            for (size_t b = a + 1; b < order.size(); ++b) {
                if (kind[b] != 65 || partner[b] >= 0 || !fixed_k(b) || !same_q(a, b)) continue;
                partner[a] = (int)b;
                partner[b] = (int)a;
                kind[a] = 72;
                kind[b] = -1;
                break;
            }
        }
    }
    // Time windows, only with DAAM_TAP_WALK=1: when the launch of the head_dim-64 chains would take the eight-wave FULL64
    // tap_d64_kernel and some layer has recorded steps in two or more of its window slots, every such chain goes to tap_walk_kernel
    // (kind 73): one table entry per LAYER that walks the layer's windows in recorded order -- a layer with one window in this flush as a
    // walk of length one, rather than a second kernel beside it.  Bit-identical sums (tests/test_gpu_tap_walk.py).
    if (c->tap_walk && c->n_bins > 1 && !c->no_w8) {
        const int kd = in_dtype == DAAM_BF16 ? 66 : 65;
        bool full64 = true, multi = false;
        std::vector<char> seen(c->max_layers, 0);
        for (size_t i = 0; i < order.size(); ++i) {
            if (kind[i] != kd) continue;
            full64 = full64 && per[i][0]->d.head_dim == 64;
            multi = multi || seen[order[i] % c->max_layers]++;
        }
        if (multi && full64 && tap_walk_has(in_dtype, c->acc_dtype) && tap_d64_tile_pixels(in_dtype, c->acc_dtype, 1) == tap_walk_tile_pixels())
            for (int& k2 : kind)
                if (k2 == kd) k2 = 73;
    }
    std::vector<int> kinds;
    for (int kd : kind)
        if (kd >= 0 && std::find(kinds.begin(), kinds.end(), kd) == kinds.end()) kinds.push_back(kd);
    int rc = 0;
    int grid_total = 0;
    // pass 1: the tables of every kernel kind -> ring -> device (all on the caller's stream)
    struct Prepared { int kd; TapLaunch L; int max_d; int min_d; int all_round; size_t ring_begin, ring_end; bool w8;
                      const WalkEntry* walk_entries; const WalkWin* walk_wins; };
    std::vector<Prepared> prepared;
    for (int kd : kinds) {
        size_t n_layers = 0, n_ptrs = 0;
        for (size_t i = 0; i < order.size(); ++i)
            if (kind[i] == kd) { ++n_layers; n_ptrs += per[i].size() * (kd == 72 ? 2 : 1); }
        int tile = kd == 73 ? tap_walk_tile_pixels() : kd == 72 ? tap_pair_tile_pixels() : kd == 71 ? tap_slab_tile_pixels() : kd ? tap_mfma_tile_pixels() : kTapPixels;
        bool w8 = false;
        if ((kd == 65 || kd == 66) && !c->no_w8) {
            // head_dim-64 launches with fp16 Q / K and fp16 sums: 256-pixel tiles on eight-wave workgroups (one K tile for twice the pixels)
            bool full64 = true;
            for (size_t i = 0; i < order.size(); ++i)
                if (kind[i] == kd) full64 = full64 && per[i][0]->d.head_dim == 64;
            const int t8 = tap_d64_tile_pixels(in_dtype, c->acc_dtype, full64 ? 1 : 0);
            w8 = t8 != tile;
            tile = t8;
        }
        if (!kd) {                                           // the generic kernel reads the sums first
            for (size_t i = 0; i < order.size() && !rc; ++i)
                if (kind[i] == kd) rc = ensure_zeroed(c->layers[order[i]], s);
            if (rc) break;
        }
        // table entries of this kind: one per layer -- except that the slab kernel (71) may take the LAST pixels of a head_dim-40 layer as a second
        // entry with 16-pixel tiles (see below)
        struct Ent { size_t i; int rank, px_begin, px_end, tile; };
        std::vector<Ent> ents;
        // walk kernel (73): entry = the window chains (indices into `order`) of one layer, in recorded order.  An entry ends where its
        // steps would pass the launch's step limit (the pointer table in LDS holds the ENTRY's steps) or where a window's shape or
        // strides differ from the entry's: the layer then has another entry for its later windows -- never a window in two entries.
        std::vector<std::vector<size_t>> walk;
        size_t n_walk_wins = 0;
        if (kd == 73) {
            std::vector<int> open(c->max_layers, -1), steps_in;
            auto same_shape = [](const DaamQKDesc& o, const DaamQKDesc& d) {
                return o.batch == d.batch && o.heads == d.heads && o.head_dim == d.head_dim && o.hw == d.hw && o.round_logits == d.round_logits &&
                       o.scale == d.scale && o.q_stride_b == d.q_stride_b && o.q_stride_h == d.q_stride_h && o.q_stride_p == d.q_stride_p &&
                       o.k_stride_b == d.k_stride_b && o.k_stride_h == d.k_stride_h && o.k_stride_t == d.k_stride_t;
            };
            for (size_t i = 0; i < order.size(); ++i) {
                if (kind[i] != kd) continue;
                const int layer = order[i] % c->max_layers;
                int e = open[layer];
                if (e < 0 || steps_in[e] + (int)per[i].size() > tap_mfma_max_steps() || !same_shape(per[walk[e][0]][0]->d, per[i][0]->d)) {
                    e = open[layer] = (int)walk.size();
                    walk.emplace_back();
                    steps_in.push_back(0);
                }
                walk[e].push_back(i);
                steps_in[e] += (int)per[i].size();
                ++n_walk_wins;
            }
            for (auto& g : walk) ents.push_back({g[0], 0, 0, per[g[0]][0]->d.hw, tile});
        }
        // slab kernel: the layers segment by segment (one cost per workgroup each): head_dim 160 first (few, light workgroups with the longest
        // step chains), 40 (the bulk), 80 (short chains), and last the TAIL of the head_dim-40 layers in half-size workgroups: 2.2 rounds of
        // indivisible 50-step chains leave a third of the chip idle for the last 100 us of the launch; half-length units empty it more evenly
        // (DAAM_SLAB_TAIL = percent of a head_dim-40 layer's pixels that go there; bit-identical sums either way).  Every XCD takes an eighth of
        // each segment.  Round 6 searched the order with a list-scheduling model (tools/slab_order_model.py) and measured its best candidate
        // ("columns": first halves heavy-first, second halves light-first, half-size units last) on the chip: 3 % SLOWER than this order for
        // every tail share (LABNOTES R6.2) -- a chain's speed depends on what shares its CU, which the model does not know.
        auto seg_rank = [](int d) { return d == 160 ? 0 : d == 40 ? 1 : 2; };
        for (size_t i = 0; i < order.size(); ++i) {
            if (kind[i] != kd || kd == 73) continue;
            const DaamQKDesc& d0 = per[i][0]->d;
            if (kd != 71) { ents.push_back({i, 0, 0, d0.hw, tile}); continue; }
            const int r = seg_rank(d0.head_dim);
            const int tail_px = (r == 1 && d0.hw >= 64) ? (int)((int64_t)d0.hw * c->slab_tail_pct / 100 / 32) * 32 : 0;
            if (d0.hw - tail_px > 0) ents.push_back({i, r, 0, d0.hw - tail_px, tile});
            if (tail_px > 0) ents.push_back({i, 3, d0.hw - tail_px, d0.hw, tile / 2});
        }
        if (kd == 71) std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.rank < b.rank; });
        n_layers = ents.size();
        // tap_pair_kernel: the chain-B entries follow the chain-A entries, one per pair, in the same order
        // tap_walk_kernel: its window table and per-entry window ranges follow the step pointers
        const size_t bytes_layers = n_layers * (kd == 72 ? 2 : 1) * sizeof(TapLayer), bytes_tap = bytes_layers + n_ptrs * sizeof(TapPtr);
        const size_t bytes = bytes_tap + n_walk_wins * sizeof(WalkWin) + walk.size() * sizeof(WalkEntry);
        size_t off = 0;
        hipError_t e = c->ring.alloc(bytes, &off);
        if (e != hipSuccess) { rc = fail((int)e, "upload ring: %s", hipGetErrorString(e)); break; }
        TapLayer* hl = reinterpret_cast<TapLayer*>(c->ring.host + off);
        TapPtr* hp = reinterpret_cast<TapPtr*>(c->ring.host + off + bytes_layers);
        WalkWin* hw_wins = reinterpret_cast<WalkWin*>(c->ring.host + off + bytes_tap);
        WalkEntry* hw_ents = reinterpret_cast<WalkEntry*>(c->ring.host + off + bytes_tap + n_walk_wins * sizeof(WalkWin));
        int wg = 0, ptr = 0, max_d = 0, min_d = 1 << 30, all_round = 1;
        std::vector<int> ptr_of(order.size(), -1);             // a layer's step pointers are written once, both of its entries point at them
        for (size_t e = 0, win = 0; e < walk.size(); ++e) {     // (73) a window's step pointers follow the previous window's
            hw_ents[e].win_begin = (int32_t)win;
            hw_ents[e].n_win = (int32_t)walk[e].size();
            for (size_t i : walk[e]) {
                const Layer& wl = c->layers[order[i]];
                hw_wins[win].acc = wl.acc;
                hw_wins[win].n_steps = (int32_t)per[i].size();
                hw_wins[win].fresh = wl.dirty ? 0 : 1;
                ++win;
                ptr_of[i] = ptr;
                for (auto* p : per[i]) { hp[ptr].q = p->q; hp[ptr].k = p->k; ++ptr; }
            }
        }
        for (size_t i = 0; i < order.size(); ++i) {
            if (kind[i] != kd || kd == 73) continue;
            for (size_t m = 0; m < (kd == 72 ? 2u : 1u); ++m) {
                const size_t ci = m ? (size_t)partner[i] : i;
                ptr_of[ci] = ptr;
                for (auto* p : per[ci]) { hp[ptr].q = p->q; hp[ptr].k = p->k; ++ptr; }
            }
        }
        size_t j = 0;
        int seg_begin[kMaxSlabSegs + 1] = {0}, n_seg = 0;
        int last_rank = -1;
        for (const Ent& en : ents) {
            const auto& v = per[en.i];
            fill_layer(c, c->layers[order[en.i]], v[0]->d, en.tile, &hl[j]);
            hl[j].wg_begin = wg;
            hl[j].n_steps = (int)v.size();
            if (kd == 73) {                                  // the entry's steps: every window's
                hl[j].n_steps = 0;
                for (size_t i : walk[j]) hl[j].n_steps += (int)per[i].size();
            }
            hl[j].ptr_begin = ptr_of[en.i];
            hl[j].px_begin = en.px_begin;
            hl[j].px_end = en.px_end;
            hl[j].tile_px = en.tile;
            hl[j].tiles_per_head = (en.px_end - en.px_begin + en.tile - 1) / en.tile;
            if (kd == 71) {
                if (en.rank != last_rank) { seg_begin[n_seg++] = wg; last_rank = en.rank; }
                wg += hl[j].heads_kept / tap_slab_heads(v[0]->d.head_dim) * hl[j].tiles_per_head;   // tiles_per_head = tiles per slab
            } else {
                wg += hl[j].heads_kept * hl[j].tiles_per_head;
            }
            max_d = std::max(max_d, v[0]->d.head_dim);
            min_d = std::min(min_d, v[0]->d.head_dim);
            all_round = all_round && v[0]->d.round_logits;
            if (kd == 72) {                                  // chain B: its own sums, fresh flag, K batch stride and pointer pair
                const size_t bi = (size_t)partner[en.i];
                TapLayer& hb = hl[n_layers + j];
                fill_layer(c, c->layers[order[bi]], per[bi][0]->d, en.tile, &hb);
                hb.wg_begin = hl[j].wg_begin;
                hb.n_steps = hl[j].n_steps;
                hb.ptr_begin = ptr_of[bi];
                hb.tiles_per_head = hl[j].tiles_per_head;
            }
            ++j;
        }
        seg_begin[n_seg] = wg;
        // daam_finalize_prepare: the output of the finalize that follows this launch is cleared by this (first) upload kernel
        const bool fold = c->fold_out && c->fold_stream == s;
        e = c->ring.commit(off, bytes, s, fold ? c->fold_out : nullptr, fold ? c->fold_bytes : 0);
        if (e != hipSuccess) { rc = fail((int)e, "table upload: %s", hipGetErrorString(e)); break; }
        if (fold) {
            c->prep_out = c->fold_out;
            c->prep_stream = s;
            c->fold_out = nullptr;
        }
        Prepared pr;
        pr.kd = kd;
        memset(&pr.L, 0, sizeof pr.L);
        pr.L.layers = reinterpret_cast<const TapLayer*>(c->ring.dev + off);
        pr.L.ptrs = reinterpret_cast<const TapPtr*>(c->ring.dev + off + bytes_layers);
        pr.L.n_layers = (int)n_layers;
        pr.L.tokens = c->tokens;
        pr.L.total_wgs = wg;
        pr.L.wgs_per_xcd = (wg + 7) / 8;
        pr.L.n_seg = n_seg;
        for (int k = 0; k <= kMaxSlabSegs; ++k) pr.L.seg_begin[k] = seg_begin[k];
        pr.max_d = max_d;
        pr.min_d = min_d;
        pr.all_round = all_round;
        pr.w8 = w8 || kd == 73;
        pr.walk_entries = reinterpret_cast<const WalkEntry*>(c->ring.dev + off + bytes_tap + n_walk_wins * sizeof(WalkWin));
        pr.walk_wins = reinterpret_cast<const WalkWin*>(c->ring.dev + off + bytes_tap);
        pr.ring_begin = c->ring.cur_begin;
        pr.ring_end = c->ring.cur_end;
        prepared.push_back(pr);
    }
    // pass 2: one launch per kind.  A flush with several kinds (SD-v1.5: head_dim 40 / 80 / 160) has kernels of a
    // few dozen to a few hundred workgroups x 50 sequential steps each, which leave most of the chip idle when run
    // one after the other.  The largest stays on the caller's stream, every other kind gets its own auxiliary
    // non-blocking stream, forked from / joined to the caller's stream by events (all tables are uploaded before
    // the fork) and launched FIRST so that its few workgroups are resident when the large grid fills the rest.
    const bool side = !rc && prepared.size() > 1 && prepared.size() <= (size_t)DaamCtx::kAux + 1 && !c->no_side_stream;
    if (side) {
        hipError_t ae = ensure_aux(c);
        if (ae != hipSuccess) rc = fail((int)ae, "auxiliary streams: %s", hipGetErrorString(ae));
    }
    size_t main_idx = 0;
    for (size_t i = 1; i < prepared.size(); ++i)
        if (prepared[i].L.total_wgs > prepared[main_idx].L.total_wgs) main_idx = i;
    const bool ev_started = c->profile && !rc && !prepared.empty();
    if (ev_started) (void)hipEventRecord(c->prof_event(0, 0), s);
    bool forked = false;
    if (side && !rc) {
        if (hipEventRecord(c->aux_fork, s) != hipSuccess) rc = fail(DAAM_E_STATE, "stream fork failed");
        else forked = true;
    }
    std::vector<size_t> launch_order;                        // side kinds first, the main one last
    for (size_t i = 0; i < prepared.size(); ++i)
        if (!forked || i != main_idx) launch_order.push_back(i);
    if (forked) launch_order.push_back(main_idx);
    int n_side = 0;
    // start gate: the side kernels' workgroups count themselves in, the main kernel waits (one wave, bounded) until they are
    // resident -- only for the kernels that carry the counter (the MFMA kinds).
    // A gate that runs into its 200 us timeout means the side kernels were NOT running beside the caller's stream at that moment (one
    // hardware queue, GPU_MAX_HW_QUEUES; or another process held the GPU): every gated flush then pays the 200 us for nothing.  The
    // timeout counter is pinned host memory the gate kernels bump; the host reads it here WITHOUT synchronising, so it lags the
    // enqueued flushes by however many are still in flight.  Rule (robust against that lag): since the gate was last armed, at least
    // three timeouts AND at least half of the gated flushes enqueued so far timed out -> the gate rests for 64 flushes (said once),
    // then is armed again with fresh counts.
    if (forked && c->gate_timeouts) {
        const unsigned now = *reinterpret_cast<volatile unsigned*>(c->gate_timeouts);
        if (c->gate_off_until && c->n_flushes >= c->gate_off_until) { c->gate_off_until = 0; c->gate_timeouts_seen = now; c->gate_enqueued = 0; }
        if (!c->gate_off_until) {
            const unsigned timeouts = now - c->gate_timeouts_seen;         // since armed (unsigned wrap-around is fine)
            if (timeouts >= 3 && 2 * (unsigned long long)timeouts >= c->gate_enqueued) {
                c->gate_off_until = c->n_flushes + 64;
                if (!c->gate_said) {
                    c->gate_said = true;
                    fprintf(stderr, "libdaam_hip: the start gate of %u of %llu multi-kernel tap launches timed out (side streams not concurrent with "
                                    "the caller's stream); the gate rests for 64 launches\n", timeouts, c->gate_enqueued);
                }
            }
        }
    }
    bool gate = forked && !c->no_start_gate && !c->gate_off_until && c->d_started;
    for (size_t i = 0; i < prepared.size(); ++i)
        if (i != main_idx && !prepared[i].kd) gate = false;
    unsigned gate_wgs = 0;
    std::string launched_names;
    for (size_t pi : launch_order) {
        if (rc) break;
        Prepared& pr = prepared[pi];
        hipStream_t ks = s;
        if (forked && pi != main_idx) {
            ks = c->aux_stream[n_side];
            if (hipStreamWaitEvent(ks, c->aux_fork, 0) != hipSuccess) { rc = fail(DAAM_E_STATE, "stream fork failed"); break; }
            if (gate) { pr.L.started = c->d_started; gate_wgs += (unsigned)pr.L.total_wgs; }
        } else if (gate && gate_wgs) {
            c->started_target += gate_wgs;                     // unsigned wrap-around is fine: the kernel compares differences
            hipError_t ge = launch_start_gate(c->d_started, c->started_target, 200, c->gate_timeouts_dev, s);
            if (ge != hipSuccess) { rc = fail((int)ge, "start gate: %s", hipGetErrorString(ge)); break; }
        }
        int grid = 0;
        WalkLaunch WL;
        if (pr.kd == 73) { WL.L = pr.L; WL.entries = pr.walk_entries; WL.wins = pr.walk_wins; }
        hipError_t e = pr.kd == 73 ? launch_tap_walk(WL, in_dtype, c->acc_dtype, c->fast_exp && pr.all_round, ks, &grid, &c->last_lds[0])
                     : (pr.kd == 65 || pr.kd == 66) ? launch_tap_d64(pr.L, in_dtype, c->acc_dtype, c->fast_exp && pr.all_round, pr.min_d == 64 && pr.max_d == 64, pr.w8 ? 1 : 0, c->tap_sync, ks, &grid, &c->last_lds[0])
                     : (pr.kd == 67 || pr.kd == 69) ? launch_tap_wide(pr.L, c->acc_dtype, pr.max_d, c->fast_exp && pr.all_round, ks, &grid, &c->last_lds[0])
                     : pr.kd == 70 ? launch_tap_chunk(pr.L, in_dtype, c->acc_dtype, c->fast_exp && pr.all_round, pr.min_d != pr.max_d, ks, &grid, &c->last_lds[0])
                     : pr.kd == 71 ? launch_tap_slab(pr.L, c->acc_dtype, c->fast_exp && pr.all_round, ks, &grid, &c->last_lds[0])
                     : pr.kd == 72 ? launch_tap_pair(pr.L, c->fast_exp && pr.all_round, ks, &grid, &c->last_lds[0])
                     : pr.kd ? launch_tap_mfma(pr.L, c->acc_dtype, pr.max_d, c->fast_exp && pr.all_round, ks, &grid, &c->last_lds[0])
                             : launch_tap_generic(pr.L, in_dtype, c->acc_dtype, pr.max_d, ks, &grid, &c->last_lds[0]);
        grid_total += grid;
        if (e != hipSuccess) { rc = fail((int)e, "tap launch: %s", hipGetErrorString(e)); break; }
        launched_names += (launched_names.empty() ? "" : "+") + std::string(tap_kernel_name(pr.kd));
        e = c->ring.release_range(pr.ring_begin, pr.ring_end, ks);
        if (e != hipSuccess) { rc = fail((int)e, "event record: %s", hipGetErrorString(e)); break; }
        if (ks != s) {
            if (hipEventRecord(c->aux_join[n_side], ks) != hipSuccess) { rc = fail(DAAM_E_STATE, "stream join failed"); break; }
            ++n_side;
        }
        for (size_t i = 0; i < order.size(); ++i)
            if (kind[i] == pr.kd || (pr.kd == 72 && kind[i] == -1)) { c->layers[order[i]].dirty = true; c->layers[order[i]].zero_pending = false; }
    }
    // a flush that failed part-way may have announced side workgroups that never started: counter and target would disagree for
    // good (every later gate a silent no-op or a full timeout), so the context stops gating
    if (rc && gate) c->no_start_gate = 1;
    if (forked && gate && gate_wgs != 0) ++c->gate_enqueued;
    // join (after the main kernel is enqueued): the caller's stream continues when every side kernel is done
    for (int i = 0; i < n_side; ++i)
        if (hipStreamWaitEvent(s, c->aux_join[i], 0) != hipSuccess) rc = rc ? rc : fail(DAAM_E_STATE, "stream join failed");
    if (c->profile && ev_started) { (void)hipEventRecord(c->prof_event(0, 1), s); ++c->hist_count[0]; }
    c->last_grid[0] = grid_total;
    c->last_block[0] = 256;
    for (auto& pr : prepared)
        if (pr.w8 || pr.kd == 71 || pr.kd == 72) c->last_block[0] = 512;
    c->last_kernels[0] = launched_names;
    c->last_flush_kernels = (int)launch_order.size();
    c->last_flush_side = n_side;
    c->last_flush_steps = 0;
    for (auto& v : per) c->last_flush_steps = std::max(c->last_flush_steps, (int)v.size());
    ++c->n_flushes;
    c->drop_pending();
    c->fold_out = nullptr;                                     // one-shot: never carried to a later launch
    return rc;
}

int daam_tap_probs(DaamCtx* c, int layer, const void* probs, int in_dtype, int batch_heads, int hw, int tokens,
                   void* stream)
{
    if (!c || !probs) return fail(DAAM_E_INVALID, "NULL argument");
    if (layer < 0 || layer >= c->max_layers || !c->layers[layer].configured)
        return fail(DAAM_E_STATE, "layer %d not configured", layer);
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "probs tap with deferred taps pending: flush first");
    const Layer& l = c->layers[layer];
    if (in_dtype != DAAM_F16 && in_dtype != DAAM_F32 && in_dtype != DAAM_BF16) return fail(DAAM_E_INVALID, "in_dtype %d", in_dtype);
    if (!dtypes_compatible(in_dtype, c->acc_dtype))
        return fail(DAAM_E_INVALID, "probabilities of dtype %d cannot feed running sums of dtype %d (own dtype or f32)", in_dtype, c->acc_dtype);
    if (tokens != c->tokens) return fail(DAAM_E_INVALID, "tokens %d != context size %d", tokens, c->tokens);
    if (batch_heads - batch_heads / 2 != l.heads || hw != l.hw)
        return fail(DAAM_E_INVALID, "layer %d is [%d heads, %d positions], call has [%d kept, %d]", layer, l.heads, l.hw,
                    batch_heads - batch_heads / 2, hw);
    DeviceGuard on_device(c);
    const int slot = c->slot_of(layer);
    {
        int zrc = ensure_zeroed(c->layers[slot], (hipStream_t)stream);
        if (zrc) return zrc;
    }
    ProbsLaunch L;
    L.acc = c->layers[slot].acc;
    L.probs = probs;
    L.heads_kept = l.heads;
    L.bh_first = batch_heads / 2;
    L.hw = hw;
    L.tokens = tokens;
    L.tiles_per_head = (hw + kTapPixels - 1) / kTapPixels;
    L.total_wgs = L.heads_kept * L.tiles_per_head;
    L.wgs_per_xcd = (L.total_wgs + 7) / 8;
    c->last_block[0] = 256;
    hipError_t e = launch_tap_probs(L, in_dtype, c->acc_dtype, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0]);
    if (e != hipSuccess) return fail((int)e, "probs tap launch: %s", hipGetErrorString(e));
    c->layers[slot].dirty = true;
    ++c->tap_steps[layer];
    return 0;
}

int daam_key_offset(DaamCtx* c, int layer, int* offset, int* total)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    int off = 0, tot = 0;
    for (int i = 0; i < c->max_layers; ++i) {
        if (i == layer) off = tot;
        if (c->layers[i].configured) tot += c->layers[i].heads;
    }
    if (offset) *offset = off;
    if (total) *total = tot;
    return 0;
}


int daam_epilogue_normalize(float* maps, int n_rows, int side, void* stream)
{
    if (!maps || n_rows <= 0 || side <= 0) return fail(DAAM_E_INVALID, "bad argument");
    hipError_t e = launch_normalize(maps, n_rows, side * side, (hipStream_t)stream);
    if (e != hipSuccess) return fail((int)e, "normalize launch: %s", hipGetErrorString(e));
    return 0;
}

int daam_word_heat_map(const float* maps, int side, const int32_t* idx, int n_idx, float* word_map, float* out,
                       int out_h, int out_w, int absolute, float threshold, float* workspace, void* stream)
{
    if (!maps || !idx || !word_map || !workspace) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_idx <= 0 || n_idx > kMaxTokens) return fail(DAAM_E_INVALID, "n_idx %d not in 1..%d", n_idx, kMaxTokens);
    if (side <= 0 || (out && (out_h <= 0 || out_w <= 0))) return fail(DAAM_E_INVALID, "bad size");
    hipError_t e = launch_word(maps, side, idx, n_idx, word_map, out, out_h, out_w, absolute, threshold, workspace,
                               (hipStream_t)stream);
    if (e != hipSuccess) return fail((int)e, "word map launch: %s", hipGetErrorString(e));
    return 0;
}

int daam_mask_overlap(const float* a, int a_h, int a_w, const float* b, int b_h, int b_w, int n_pairs, float* sums, void* stream)
{
    if (!a || !b || !sums) return fail(DAAM_E_INVALID, "NULL argument");
    if (n_pairs <= 0 || n_pairs > 65535 || a_h <= 0 || a_w <= 0 || b_h <= 0 || b_w <= 0 || (long long)b_h * b_w > (1ll << 30))
        return fail(DAAM_E_INVALID, "bad shape: %d pairs, a %dx%d, b %dx%d", n_pairs, a_h, a_w, b_h, b_w);
    if (a_h == b_h && a_w != b_w)
        return fail(DAAM_E_INVALID, "same heights but widths %d / %d differ (the reference's a * b would not broadcast)", a_w, b_w);
    hipError_t e = launch_mask_overlap(a, a_h, a_w, b, b_h, b_w, n_pairs, sums, (hipStream_t)stream);
    if (e != hipSuccess) return fail((int)e, "mask overlap launch: %s", hipGetErrorString(e));
    return 0;
}

int daam_profile_enable(DaamCtx* c, int on)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    DeviceGuard on_device(c);
    if (on && !c->prof_ev[0][0])
        for (auto& pair : c->prof_ev)
            for (auto& ev : pair) HIP_TRY(hipEventCreate(&ev));

    if (on == 2) {
        for (int which = 0; which < 2; ++which)
            for (int end = 0; end < 2; ++end)
                if (c->hist_ev[which][end].empty()) {
                    std::vector<hipEvent_t> ring(DaamCtx::kProfHist, nullptr);
                    hipError_t e = hipSuccess;
                    for (auto& ev : ring)
                        if ((e = hipEventCreate(&ev)) != hipSuccess) break;
                    if (e != hipSuccess) {                     // never leave a ring with null events behind: prof_event() would hand them out
                        for (auto ev : ring)
                            if (ev) (void)hipEventDestroy(ev);
                        return fail((int)e, "profile event ring: %s", hipGetErrorString(e));
                    }
                    c->hist_ev[which][end] = std::move(ring);
                }
        c->hist_count[0] = c->hist_count[1] = 0;
    }
    c->profile = on == 2 ? 2 : on ? 1 : 0;
    return 0;
}

int daam_profile_history(DaamCtx* c, int which, float* ms, int capacity, int* n)
{
    if (!c || !ms || !n || which < 0 || which > 1 || capacity < 0) return fail(DAAM_E_INVALID, "bad argument");
    if (c->hist_ev[which][0].empty()) return fail(DAAM_E_STATE, "daam_profile_enable(ctx, 2) was never called");
    DeviceGuard on_device(c);
    const long long have = std::min<long long>(c->hist_count[which], DaamCtx::kProfHist);
    const int take = (int)std::min<long long>(have, capacity);
    *n = take;
    for (int i = 0; i < take; ++i) {                       // oldest of the last `take` launches first
        const size_t slot = (size_t)((c->hist_count[which] - take + i) % DaamCtx::kProfHist);
        HIP_TRY(hipEventSynchronize(c->hist_ev[which][1][slot]));
        HIP_TRY(hipEventElapsedTime(&ms[i], c->hist_ev[which][0][slot], c->hist_ev[which][1][slot]));
    }
    return 0;
}

int daam_profile_last_ms(DaamCtx* c, int which, float* ms)
{
    if (!c || !ms || which < 0 || which > 1) return fail(DAAM_E_INVALID, "bad argument");
    if (!c->prof_ev[which][0]) return fail(DAAM_E_STATE, "profiling was never enabled");
    DeviceGuard on_device(c);
    if (c->profile == 2) {                                     // the launches record into the ring: the newest slot, not a stale prof_ev pair
        if (c->hist_count[which] <= 0 || c->hist_ev[which][0].empty()) return fail(DAAM_E_STATE, "no launch of kind %d since daam_profile_enable(ctx, 2)", which);
        const size_t slot = (size_t)((c->hist_count[which] - 1) % DaamCtx::kProfHist);
        HIP_TRY(hipEventSynchronize(c->hist_ev[which][1][slot]));
        HIP_TRY(hipEventElapsedTime(ms, c->hist_ev[which][0][slot], c->hist_ev[which][1][slot]));
        return 0;
    }
    HIP_TRY(hipEventSynchronize(c->prof_ev[which][1]));
    HIP_TRY(hipEventElapsedTime(ms, c->prof_ev[which][0], c->prof_ev[which][1]));
    return 0;
}

int daam_clock_monitor_start(DaamCtx* c, int n_samples, int period_us)
{
    if (!c || n_samples < 2 || n_samples > kClockMaxSamples || period_us < 1) return fail(DAAM_E_INVALID, "bad argument");
    DeviceGuard on_device(c);
    if (!c->clk_host) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->clk_host), 2 * kClockMaxSamples * sizeof(unsigned long long), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->clk_dev), c->clk_host, 0));
        HIP_TRY(hipStreamCreateWithFlags(&c->clk_stream, hipStreamNonBlocking));
    }
    HIP_TRY(hipStreamSynchronize(c->clk_stream));
    memset(c->clk_host, 0, 2 * kClockMaxSamples * sizeof(unsigned long long));
    c->clk_samples = n_samples;
    hipError_t e = launch_clock_monitor(c->clk_dev, n_samples, period_us, c->clk_stream);
    if (e != hipSuccess) return fail((int)e, "clock monitor launch: %s", hipGetErrorString(e));
    return 0;
}

int daam_clock_monitor_read(DaamCtx* c, float* mhz, int capacity, int* n_intervals)
{
    if (!c || !mhz || !n_intervals) return fail(DAAM_E_INVALID, "NULL argument");
    if (!c->clk_host || c->clk_samples < 2) return fail(DAAM_E_STATE, "the clock monitor was never started");
    DeviceGuard on_device(c);
    HIP_TRY(hipStreamSynchronize(c->clk_stream));
    int n = 0;
    for (int i = 1; i < c->clk_samples && n < capacity; ++i) {
        const unsigned long long* a = c->clk_host + 2 * (i - 1), *b = c->clk_host + 2 * i;
        if (b[1] > a[1] && b[0] > a[0]) mhz[n++] = (float)((double)(b[0] - a[0]) / (double)(b[1] - a[1]) * 100.0);   // reference: 100 MHz
    }
    *n_intervals = n;
    return 0;
}

int daam_last_flush(DaamCtx* c, int* n_kernels, int* n_side_streams, int* max_steps, long long* n_flushes)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    if (n_kernels) *n_kernels = c->last_flush_kernels;
    if (n_side_streams) *n_side_streams = c->last_flush_side;
    if (max_steps) *max_steps = c->last_flush_steps;
    if (n_flushes) *n_flushes = c->n_flushes;
    return 0;
}

int daam_last_kernels(DaamCtx* c, int which, char* names, int capacity)
{
    if (!c || !names || capacity <= 0 || which < 0 || which > 1) return fail(DAAM_E_INVALID, "bad argument");
    snprintf(names, (size_t)capacity, "%s", c->last_kernels[which].c_str());
    return 0;
}

int daam_last_launch(DaamCtx* c, int which, int* grid, int* block, int* lds_bytes)
{
    if (!c || which < 0 || which > 1) return fail(DAAM_E_INVALID, "bad argument");
    if (grid) *grid = c->last_grid[which];
    if (block) *block = c->last_block[which];
    if (lds_bytes) *lds_bytes = c->last_lds[which];
    return 0;
}

}  // extern "C"
