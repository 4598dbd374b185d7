// Host side of libdaam_hip.so: the C ABI declared in include/daam_hip.h -- context, layers, time bins, attend, probs tap,
// profiling and the clock monitor (the tap entry points: daam_tap_api.hip; the finalize ones: daam_finalize_api.hip; the epilogue's:
// daam_epilogue.hip and the three files beside it).
// Owns no activations; owns (optionally) the running sums, the bicubic tap tables and a
// small pinned upload ring for the per-launch device tables.
#include "daam_ctx.h"

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

int launched(const char* what, hipError_t e)
{
    return e == hipSuccess ? 0 : fail((int)e, "%s launch: %s", what, hipGetErrorString(e));
}

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

// The (h, w) table pair of finalize_rect_kernel: bicubic_table(w, out_w) for the row pass, bicubic_table(h, out_h) for the
// column pass, one pair per distinct (h, w) of the context (as tab_sides for the square classes).
int rect_tab(DaamCtx* c, Layer& l)
{
    if (l.rtab != -2) return 0;
    if (l.h == c->out_h && l.w == c->out_w) { l.rtab = -1; return 0; }
    for (size_t i = 0; i < c->rtab_hw.size(); ++i)
        if (c->rtab_hw[i] == std::make_pair(l.h, l.w)) { l.rtab = (int)i; return 0; }
    if ((int)c->rtab_hw.size() >= kMaxTabs) return fail(DAAM_E_UNSUPPORTED, "more than %d distinct map sizes", kMaxTabs);
    const size_t per = (size_t)(c->out_w + c->out_h) * 4;
    if (!c->d_rtab_idx) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_rtab_idx), sizeof(int16_t) * kMaxTabs * per));
    if (!c->d_rtab_w) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_rtab_w), sizeof(float) * kMaxTabs * per));
    const int tab = (int)c->rtab_hw.size();
    std::vector<int16_t> idx(per);
    std::vector<float> w(per);
    bicubic_table(l.w, c->out_w, idx.data(), w.data());
    bicubic_table(l.h, c->out_h, idx.data() + (size_t)c->out_w * 4, w.data() + (size_t)c->out_w * 4);
    HIP_TRY(hipMemcpy(c->d_rtab_idx + tab * per, idx.data(), per * sizeof(int16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_rtab_w + tab * per, w.data(), per * sizeof(float), hipMemcpyHostToDevice));
    c->rtab_hw.push_back({l.h, l.w});
    l.rtab = tab;
    return 0;
}

extern "C" {

int daam_abi_version(void) { return DAAM_ABI_VERSION; }
const char* daam_last_error(void) { return g_err.c_str(); }

int daam_ctx_create(int max_layers, int tokens, int out_side, int acc_dtype, DaamCtx** out)
{
    if (out && (out_side <= 0 || out_side > 128)) {
        *out = nullptr;
        return fail(DAAM_E_INVALID, "out_side %d not in 1..128", out_side);
    }
    return daam_ctx_create_rect(max_layers, tokens, out_side, out_side, acc_dtype, out);
}

int daam_ctx_create_rect(int max_layers, int tokens, int out_h, int out_w, int acc_dtype, DaamCtx** out)
{
    if (!out) return fail(DAAM_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_layers <= 0 || max_layers > 4096) return fail(DAAM_E_INVALID, "max_layers %d out of range", max_layers);
    if (tokens <= 0 || tokens > kMaxTokens) return fail(DAAM_E_INVALID, "tokens %d not in 1..%d", tokens, kMaxTokens);
    if (out_h <= 0 || out_h > 128 || out_w <= 0 || out_w > 128) return fail(DAAM_E_INVALID, "output %d x %d not in 1..128 per side", out_h, out_w);
    const int out_side = out_h == out_w ? out_h : 0;           // 0: no square class kernel, no square table applies
    if (acc_dtype != DAAM_F16 && acc_dtype != DAAM_F32 && acc_dtype != DAAM_BF16) return fail(DAAM_E_INVALID, "acc_dtype %d", acc_dtype);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail((int)hipErrorNoDevice, "no HIP device");
    DaamCtx* c = new DaamCtx();
    HIP_TRY(hipGetDevice(&c->device));
    c->max_layers = max_layers;
    c->tokens = tokens;
    c->out_side = out_side;
    c->out_h = out_h;
    c->out_w = out_w;
    c->acc_dtype = acc_dtype;
    c->layers.resize(max_layers);
    c->tap_steps.assign(max_layers, 0);
    hipError_t e = c->ring.init();
    if (e == hipSuccess && out_side) e = hipMalloc(reinterpret_cast<void**>(&c->d_tab_idx), sizeof(int16_t) * kMaxTabs * out_side * 4);
    if (e == hipSuccess && out_side) e = hipMalloc(reinterpret_cast<void**>(&c->d_tab_w), sizeof(float) * kMaxTabs * out_side * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_fin_tab), DaamCtx::kFinTabCap);
    if (e != hipSuccess) {
        daam_ctx_destroy(c);
        return fail((int)e, "context allocation: %s", hipGetErrorString(e));
    }
    // A/B and debugging switches, read once per context: `field` = `value` when the variable's first character is `match`, else !value
    static const struct { const char* name; int DaamCtx::*field; char match; int value; } kSwitches[] = {
        {"DAAM_FORCE_GENERIC", &DaamCtx::force_generic, '1', 1},
        {"DAAM_NO_MFMA_FINALIZE", &DaamCtx::no_mfma_finalize, '1', 1},
        {"DAAM_NO_FOLD_SAME", &DaamCtx::no_fold_same, '1', 1},
        {"DAAM_NO_START_GATE", &DaamCtx::no_start_gate, '1', 1},
        {"DAAM_NO_PIPE_FINALIZE", &DaamCtx::no_pipe_finalize, '1', 1},
        {"DAAM_NO_PAIRED_FINALIZE", &DaamCtx::no_paired_finalize, '1', 1},
        {"DAAM_TAP_W8", &DaamCtx::no_w8, '0', 1},
        {"DAAM_TAP_SYNC", &DaamCtx::tap_sync, '0', 0},            // 0: the head_dim-64 tap's step protocol before the counted waits
        {"DAAM_NO_FIN_CACHE", &DaamCtx::no_fin_cache, '1', 1},
        {"DAAM_NO_D64", &DaamCtx::no_d64, '1', 1},                // debugging: 32x32-tile kernel also for head_dim 64
        {"DAAM_NO_SIDE_STREAM", &DaamCtx::no_side_stream, '1', 1},   // debugging / A-B: every tap kernel of a flush on the caller's stream
        {"DAAM_TAP_SLAB", &DaamCtx::tap_slab, '0', 0},
        {"DAAM_TAP_PAIR", &DaamCtx::no_tap_pair, '1', 0},         // 1: chains that share Q pair up on tap_pair_kernel; default: separate chains
        {"DAAM_TAP_WALK", &DaamCtx::tap_walk, '1', 1},            // 1: a layer's time windows walk through one workgroup chain (tap_walk_kernel)
        // softmax flavour of the MFMA tap: fast (default; exponent by one mixed-precision FMA, ~1e-6 relative,
        // same deviation class as the f32 summation order of q.k -- DESIGN.md section 3.1) or compensated
        // (DAAM_STRICT_EXP=1: ~1 ulp f32 like the reference's expf)
        {"DAAM_STRICT_EXP", &DaamCtx::fast_exp, '1', 0},
    };
    for (const auto& sw : kSwitches) {
        const char* v = getenv(sw.name);
        c->*sw.field = (v && v[0] == sw.match) ? sw.value : !sw.value;
    }
    const char* stl = getenv("DAAM_SLAB_TAIL");
    if (stl && stl[0]) c->slab_tail_pct = std::max(0, std::min(100, atoi(stl)));
    const char* tck = getenv("DAAM_TAP_CHUNKED");           // daam_tap_chunk.hip: unset = launches that mix head dims, 1 = always, 0 = never
    c->tap_chunked = !tck ? 2 : tck[0] == '1' ? 1 : tck[0] == '0' ? 0 : 2;
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
    if (c->d_rtab_idx) (void)hipFree(c->d_rtab_idx);
    if (c->d_rtab_w) (void)hipFree(c->d_rtab_w);
    if (c->bin_scratch) (void)hipFree(c->bin_scratch);
    delete c;
    return 0;
}

int daam_layer_configure(DaamCtx* c, int layer, int heads, int side, int factor, void* acc)
{
    if (c && layer >= 0 && layer < c->max_layers && (heads <= 0 || side <= 0 || side > 1024))
        return fail(DAAM_E_INVALID, "heads %d / side %d", heads, side);
    return daam_layer_configure_rect(c, layer, heads, side, side, factor, acc);
}

int daam_layer_configure_rect(DaamCtx* c, int layer, int heads, int h, int w, int factor, void* acc)
{
    if (!c) return fail(DAAM_E_INVALID, "ctx is NULL");
    if (layer < 0 || layer >= c->max_layers) return fail(DAAM_E_INVALID, "layer %d out of range", layer);
    if (heads <= 0 || h <= 0 || h > 1024 || w <= 0 || w > 1024) return fail(DAAM_E_INVALID, "heads %d / %d x %d positions", heads, h, w);
    if (h != w && c->n_bins > 1) return fail(DAAM_E_UNSUPPORTED, "a layer of %d x %d positions on a time-binned context", h, w);
    const int side = h == w ? h : 0;
    DeviceGuard on_device(c);
    for (auto& p : c->pending)
        if (p.layer % c->max_layers == layer) return fail(DAAM_E_STATE, "layer %d re-configured with un-flushed taps pending", layer);
    Layer& l = c->layers[layer];
    if (l.owned && l.acc) { HIP_TRY(hipFree(l.acc)); }
    l = Layer();
    l.heads = heads;
    l.side = side;
    l.h = h;
    l.w = w;
    l.hw = h * w;
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
    if (h != w || c->out_h != c->out_w) {                      // finalize_rect_kernel's tables; none of the square classes applies
        int rc = rect_tab(c, l);
        if (rc) return rc;
    } else if (side != c->out_side) {
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
    if (c->out_h != c->out_w) return fail(DAAM_E_UNSUPPORTED, "time windows on a context with a %d x %d output", c->out_h, c->out_w);
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
