// Tap half of the host API: daam_tap_qk (immediate), daam_tap_qk_enqueue / _enqueue_many / daam_tap_pending / daam_tap_flush (deferred).
// A flush reads top to bottom as  tap_group (pending calls -> chains)  ->  tap_route (the re-routing rules)  ->  tap_tables per kind
// (entries, byte layout, upload)  ->  fork / gate / launch / join  ->  bookkeeping.  Which kernel runs a chain is a TapKind; the one
// place that turns a kind into a launch_tap_*() call is tap_launch_kind(), shared by the immediate and the deferred path.
#include "daam_ctx.h"
#include "daam_tap_walk.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---- kernel kinds ---------------------------------------------------------------------------------------------------------------
enum class TapRoute { Generic, Mfma, D64, Wide, Chunk, Slab, Pair, Walk };

// One launch per distinct kind (==), kinds in first-seen order.
struct TapKind {
    TapRoute route = TapRoute::Generic;    // Generic: the any-shape kernel
    int ksteps = 0;                        // Mfma: 16-element k-steps ceil(d / 16), 1..10; Wide: 32-element k-steps, 3 (d <= 96) or 5 -- a launch per count
    bool bf16 = false;                     // D64: the bf16 form
    bool operator==(const TapKind& o) const { return route == o.route && ksteps == o.ksteps && bf16 == o.bf16; }
    bool is(TapRoute r) const { return route == r; }
    bool d64_f16() const { return route == TapRoute::D64 && !bf16; }
    bool tile16() const { return route == TapRoute::D64 || route == TapRoute::Wide; }   // the 16x16-tile kernels a mixed launch hands to the chunked one
};

const char* tap_kernel_name(const TapKind& kind)
{
    static const char* const names[] = {"tap_generic_kernel", "tap_mfma_kernel", "tap_d64_kernel", "tap_wide_kernel",
                                        "tap_chunk_kernel", "tap_slab_kernel", "tap_pair_kernel", "tap_walk_kernel"};   // TapRoute order
    return names[(int)kind.route];
}

// pixels per workgroup tile (D64: of the four-wave form; the eight-wave decision is tap_tables')
int tap_tile_pixels(const TapKind& kind)
{
    return kind.is(TapRoute::Generic) ? kTapPixels : kind.is(TapRoute::Slab) ? tap_slab_tile_pixels() : kind.is(TapRoute::Pair) ? tap_pair_tile_pixels()
           : kind.is(TapRoute::Walk) ? tap_walk_tile_pixels() : tap_mfma_tile_pixels();
}

// One kind's launch: the argument block (deferred: its tables are uploaded and `L` points at them) and what the launcher asks beside it.
struct TapTables {
    TapKind kind;
    TapLaunch L;
    int in_dtype = 0;
    int min_d = 1 << 30, max_d = 0;        // smallest / largest head_dim among its layers
    int all_round = 1;                     // every layer rounds its logits (with the context's switch: the fast softmax)
    bool w8 = false;                       // D64: eight-wave workgroups (the tiles were sized for them)
    const WalkEntry* walk_entries = nullptr;   // Walk: the tables behind the step pointers
    const WalkWin* walk_wins = nullptr;
    size_t ring_begin = 0, ring_end = 0;   // its region of the upload ring
    bool block512() const { return w8 || kind.is(TapRoute::Walk) || kind.is(TapRoute::Slab) || kind.is(TapRoute::Pair); }
};

// The single switch from a kind to its launcher.  The immediate path is its n_layers == 1, min_d == max_d, four-wave case.
hipError_t tap_launch_kind(const DaamCtx* c, const TapTables& t, hipStream_t s, int* grid, int* lds)
{
    const TapLaunch& L = t.L;
    const int in = t.in_dtype, acc = c->acc_dtype, fast = c->fast_exp && t.all_round;
    switch (t.kind.route) {
    case TapRoute::Generic: return launch_tap_generic(L, in, acc, t.max_d, s, grid, lds);
    case TapRoute::Mfma: return launch_tap_mfma(L, acc, t.max_d, fast, s, grid, lds);
    case TapRoute::D64: return launch_tap_d64(L, in, acc, fast, t.min_d == 64 && t.max_d == 64, t.w8 ? 1 : 0, c->tap_sync, s, grid, lds);
    case TapRoute::Wide: return launch_tap_wide(L, acc, t.max_d, fast, s, grid, lds);
    case TapRoute::Chunk: return launch_tap_chunk(L, in, acc, fast, t.min_d != t.max_d, s, grid, lds);
    case TapRoute::Slab: return launch_tap_slab(L, acc, fast, s, grid, lds);
    case TapRoute::Pair: return launch_tap_pair(L, fast, s, grid, lds);
    case TapRoute::Walk: return launch_tap_walk(WalkLaunch{L, t.walk_entries, t.walk_wins}, in, acc, fast, s, grid, lds);
    }
    return hipErrorInvalidValue;
}

// ---- which kernel can take a call -------------------------------------------------------------------------------------------------
// every field of two recorded calls that a table entry shares: shape, softmax flavour and strides
bool same_call_shape(const DaamQKDesc& a, const DaamQKDesc& b)
{
    return a.batch == b.batch && a.heads == b.heads && a.head_dim == b.head_dim && a.hw == b.hw && a.round_logits == b.round_logits &&
           a.scale == b.scale && a.q_stride_b == b.q_stride_b && a.q_stride_h == b.q_stride_h && a.q_stride_p == b.q_stride_p &&
           a.k_stride_b == b.k_stride_b && a.k_stride_h == b.k_stride_h && a.k_stride_t == b.k_stride_t;
}

void fill_layer(const Layer& l, const DaamQKDesc& d, int tile_pixels, TapLayer* t)
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
}

bool use_d64_bf16(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k);
bool use_chunk(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k);

bool use_mfma(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (c->force_generic) return false;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return false;
    if (d.in_dtype == DAAM_BF16) return use_d64_bf16(c, d, q, k) || use_chunk(c, d, q, k);
    return tap_mfma_supported(d, q, k);
}

// The specialised tap kernels address Q and K with 32-bit BYTE offsets from the tensor pointers: every element a call can
// address -- (batch - 1) * stride_b + (heads - 1) * stride_h + (rows - 1) * row stride + head_dim -- must stay below 2^30 elements
// (views into a large fused buffer with unusual strides fall back to the any-shape kernel instead of wrapping).
bool offsets_fit_32(const DaamQKDesc& d)
{
    const int64_t lim = (int64_t)1 << 30;
    const int64_t s[] = {d.q_stride_b, d.q_stride_h, d.q_stride_p, d.k_stride_b, d.k_stride_h, d.k_stride_t};
    for (int64_t v : s)
        if (v < 0 || v >= lim) return false;
    const int64_t q_max = (int64_t)(d.batch - 1) * d.q_stride_b + (int64_t)(d.heads - 1) * d.q_stride_h + (int64_t)(d.hw - 1) * d.q_stride_p + d.head_dim;
    const int64_t k_max = (int64_t)(d.batch - 1) * d.k_stride_b + (int64_t)(d.heads - 1) * d.k_stride_h + (int64_t)(d.tokens - 1) * d.k_stride_t + d.head_dim;
    return q_max < lim && k_max < lim;
}

bool use_d64(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return !c->no_d64 && offsets_fit_32(d) && tap_d64_supported(d, q, k);
}

// bf16 pipelines: only the 16x16-tile kernel has a bf16 variant (head_dim <= 64, 77 tokens, bf16-rounded logits);
// everything else of a bf16 pipeline runs on the any-shape kernel
bool use_d64_bf16(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return d.in_dtype == DAAM_BF16 && !c->no_d64 && c->fast_exp && d.round_logits && d.tokens == 77 && d.hw % 8 == 0 && offsets_fit_32(d) &&
           tap_d64_supported(d, q, k);
}

// 64 < head_dim <= 160 on fp16 pipelines (SD-v1.5's 80 / 160): the 16x16-tile kernel with 3 or 5 k-steps (daam_tap_wide.hip)
bool use_wide(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    return !c->no_d64 && (c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32) && offsets_fit_32(d) &&
           (int64_t)d.batch * d.q_stride_b < ((int64_t)1 << 30) && tap_wide_supported(d, q, k);
}

// the chunked kernel (daam_tap_chunk.hip) can take this call: fp16 layers of any head_dim (multiple of 8, <= 256), and bf16 layers (bf16
// or f32 sums, bf16-rounded logits, the fast softmax -- what the bf16 head_dim-64 kernel asks for; validated on the chip in round 4)
bool chunk_ok(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (!c->tap_chunked || c->no_d64 || c->force_generic || d.tokens != 77 || !offsets_fit_32(d)) return false;
    if (d.in_dtype == DAAM_BF16) {
        if (!c->fast_exp || !d.round_logits || !(c->acc_dtype == DAAM_BF16 || c->acc_dtype == DAAM_F32)) return false;
    } else if (!(c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32)) {
        return false;
    }
    return tap_chunk_supported(d, q, k);
}

// the slab kernel (daam_tap_slab.hip) can take this deferred call: fp16 Q / K, fp16 or f32 sums, head_dim 40 / 80 / 160 with the heads
// adjacent in the rows
bool slab_ok(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (!c->tap_slab || c->no_d64 || c->force_generic || d.tokens != 77 || d.in_dtype != DAAM_F16 || !offsets_fit_32(d)) return false;
    if (!(c->acc_dtype == DAAM_F16 || c->acc_dtype == DAAM_F32)) return false;
    return tap_slab_supported(d, q, k);
}

// DAAM_TAP_CHUNKED=1: every such call.  Default (2): the deferred launches that mix head dims (route_mixed_dims), and bf16 layers with
// head_dim > 64 -- no other MFMA kernel has a bf16 form for them (the any-shape kernel is ~45x slower per step).
bool use_chunk(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (c->tap_chunked == 1) return chunk_ok(c, d, q, k);
    return c->tap_chunked == 2 && d.in_dtype == DAAM_BF16 && d.head_dim > 64 && chunk_ok(c, d, q, k);
}

// kernel choice for a call use_mfma() accepts: the 16x16-tile head_dim-64 kernel by default for d <= 64, the wide one up to 160,
// else the 32x32-tile MFMA kernel
TapKind mfma_kind(const DaamCtx* c, const DaamQKDesc& d, const void* q, const void* k)
{
    if (use_chunk(c, d, q, k)) return {TapRoute::Chunk};
    if (d.in_dtype == DAAM_BF16) return {TapRoute::D64, 0, true};   // only reached when use_d64_bf16() holds
    if (use_d64(c, d, q, k)) return {TapRoute::D64};
    if (use_wide(c, d, q, k)) return {TapRoute::Wide, d.head_dim <= 96 ? 3 : 5};
    return {TapRoute::Mfma, tap_mfma_ksteps(d.head_dim)};
}

// ---- stage 1: pending calls -> chains -----------------------------------------------------------------------------------------------
// The recorded steps of one slot (a layer, or a (window, layer) slot of a binned context), in recorded order; chains in first-seen order.
struct TapChain {
    int slot = 0;
    std::vector<const Pending*> steps;
    TapKind kind;
    int partner = -1;                      // Pair: the other chain of the pair
    bool rides = false;                    // chain B of a pair: no table entry of its own kind, it rides with its chain A (`partner`)
    const DaamQKDesc& d() const { return steps[0]->d; }
};

// A chain takes a specialised kernel when every step passes use_mfma(), and then the kind of its first step.  (No "the steps disagree
// on the kind" case: the steps of a slot share every descriptor field -- enqueue_slot, check_qk -- and the predicates depend on the
// pointers only through 16-byte alignment, which use_mfma() has tested.)
std::vector<TapChain> tap_group(const DaamCtx* c)
{
    std::vector<TapChain> chains;
    std::vector<int> chain_of(c->layers.size(), -1);
    for (const Pending& p : c->pending) {
        if (chain_of[p.layer] < 0) {
            chain_of[p.layer] = (int)chains.size();
            chains.emplace_back();
            chains.back().slot = p.layer;
        }
        chains[chain_of[p.layer]].steps.push_back(&p);
    }
    for (TapChain& ch : chains) {
        bool mfma = true;
        for (const Pending* p : ch.steps) mfma = mfma && use_mfma(c, p->d, p->q, p->k);
        if (mfma) ch.kind = mfma_kind(c, ch.d(), ch.steps[0]->q, ch.steps[0]->k);
    }
    return chains;
}

// every layer of the kind has head_dim 64 (the FULL64 forms of tap_d64_kernel; what the eight-wave form and the walk kernel ask)
bool all_head_dim_64(const std::vector<TapChain>& chains, const TapKind& kind)
{
    for (const TapChain& ch : chains)
        if (ch.kind == kind && ch.d().head_dim != 64) return false;
    return true;
}

// ---- stage 2: the re-routing rules, in this order -------------------------------------------------------------------------------
// A launch that mixes head dims (SD-v1.5: 40 / 80 / 160 = the head_dim-64 kernel and the two wide ones side by side, whose LDS
// footprints keep them from sharing CUs): every such layer on the chunked kernel instead -- ONE kind of workgroup, one launch,
// no side streams, bit-identical sums (tests/test_gpu_chunked.py; +11 ... 13 % heat maps / s on the SD-v1.5 workload).
void route_mixed_dims(const DaamCtx* c, std::vector<TapChain>& chains)
{
    if (c->tap_chunked != 2) return;
    bool d64 = false, wide3 = false, wide5 = false;
    bool d64_bf16 = false, chunk = false;                      // bf16 pipelines: head_dim <= 64 -> D64 bf16, wider heads -> Chunk (use_chunk)
    for (const TapChain& ch : chains) {
        d64 = d64 || ch.kind.d64_f16();
        wide3 = wide3 || ch.kind == TapKind{TapRoute::Wide, 3};
        wide5 = wide5 || ch.kind == TapKind{TapRoute::Wide, 5};
        d64_bf16 = d64_bf16 || ch.kind == TapKind{TapRoute::D64, 0, true};
        chunk = chunk || ch.kind.is(TapRoute::Chunk);
    }
    if (!((int)d64 + (int)wide3 + (int)wide5 >= 2 || (d64_bf16 && chunk))) return;   // (an SDXL launch -- one kind -- never gets past here: no per-call checks)
    for (const TapChain& ch : chains)
        if (ch.kind.tile16())
            for (const Pending* p : ch.steps)
                if (!chunk_ok(c, p->d, p->q, p->k)) return;
    for (TapChain& ch : chains)
        if (ch.kind.tile16()) ch.kind = {TapRoute::Chunk};
}

// fp16 layers of head_dim 40 / 80 / 160 (SD-v1.x) whose every recorded step qualifies: the slab kernel -- whole 128-byte lines of Q,
// ONE launch for the three head dims (bit-identical sums: tests/test_gpu_slab.py).  DAAM_TAP_CHUNKED=0 / 1 pin the older kernels.
void route_slab(const DaamCtx* c, std::vector<TapChain>& chains, int in_dtype)
{
    if (!(c->tap_slab && c->tap_chunked == 2 && in_dtype == DAAM_F16)) return;
    for (TapChain& ch : chains) {
        if (!(ch.kind.d64_f16() || ch.kind.is(TapRoute::Wide) || ch.kind.is(TapRoute::Chunk)) || !tap_slab_heads(ch.d().head_dim)) continue;
        bool ok = true;
        for (const Pending* p : ch.steps) ok = ok && slab_ok(c, p->d, p->q, p->k);
        if (ok) ch.kind = {TapRoute::Slab};
    }
}

// Chains that read the same recorded Q (probes): head_dim-64 fp16 chains with fp16 sums pair up on tap_pair_kernel -- chain A
// any such chain, chain B one whose K is the same pointer at every step (a probe); in recorded order: generation + probe 0, probe 1 +
// probe 2, ...  The partner rides with its chain A.  Unpaired chains keep their kernel.  Only with DAAM_TAP_PAIR=1: measured slower
// than separate chains for one and two probes, 4 % faster for four, so separate chains are the default.
void route_pair(const DaamCtx* c, std::vector<TapChain>& chains, int in_dtype)
{
    if (!(!c->no_tap_pair && !c->no_w8 && in_dtype == DAAM_F16 && c->acc_dtype == DAAM_F16)) return;
    auto fixed_k = [](const TapChain& b) {
        for (const Pending* p : b.steps) if (p->k != b.steps[0]->k) return false;
        return true;
    };
    auto same_q = [&](const TapChain& a, const TapChain& b) {
        if (a.steps.size() != b.steps.size()) return false;
        DaamQKDesc y = b.d();
        y.k_stride_b = a.d().k_stride_b;                       // the one stride chain B keeps to itself (its entry carries it)
        if (a.d().head_dim != 64 || !same_call_shape(a.d(), y) || c->layers[a.slot].heads != c->layers[b.slot].heads) return false;
        for (size_t st = 0; st < a.steps.size(); ++st) if (a.steps[st]->q != b.steps[st]->q) return false;
        return true;
    };
    for (size_t a = 0; a < chains.size(); ++a) {
        if (!chains[a].kind.d64_f16() || chains[a].partner >= 0) continue;
        for (size_t b = a + 1; b < chains.size(); ++b) {
            if (!chains[b].kind.d64_f16() || chains[b].partner >= 0 || !fixed_k(chains[b]) || !same_q(chains[a], chains[b])) continue;
            chains[a].partner = (int)b;
            chains[b].partner = (int)a;
            chains[a].kind = chains[b].kind = {TapRoute::Pair};
            chains[b].rides = true;
            break;
        }
    }
}

// Time windows, only with DAAM_TAP_WALK=1: when the launch of the head_dim-64 chains would take the eight-wave FULL64
// tap_d64_kernel and some layer has recorded steps in two or more of its window slots, every such chain goes to tap_walk_kernel:
// one table entry per LAYER that walks the layer's windows in recorded order -- a layer with one window in this flush as a
// walk of length one, rather than a second kernel beside it.  Bit-identical sums (tests/test_gpu_tap_walk.py).
void route_walk(const DaamCtx* c, std::vector<TapChain>& chains, int in_dtype)
{
    if (!(c->tap_walk && c->n_bins > 1 && !c->no_w8)) return;
    const TapKind d64{TapRoute::D64, 0, in_dtype == DAAM_BF16};
    bool multi = false;
    std::vector<char> seen(c->max_layers, 0);
    for (const TapChain& ch : chains)
        if (ch.kind == d64) multi = multi || seen[ch.slot % c->max_layers]++;
    if (multi && all_head_dim_64(chains, d64) && tap_d64_has_waves8(in_dtype, c->acc_dtype) &&
        tap_d64_tile_pixels(in_dtype, c->acc_dtype, 1) == tap_walk_tile_pixels())
        for (TapChain& ch : chains)
            if (ch.kind == d64) ch.kind = {TapRoute::Walk};
}

void tap_route(const DaamCtx* c, std::vector<TapChain>& chains, int in_dtype)
{
    route_mixed_dims(c, chains);
    route_slab(c, chains, in_dtype);
    route_pair(c, chains, in_dtype);
    route_walk(c, chains, in_dtype);
}

// ---- stage 3: one kind's device tables ------------------------------------------------------------------------------------------------
// Table entries of a kind: one per chain -- except that the slab kernel may take the LAST pixels of a head_dim-40 layer as a second entry
// with 16-pixel tiles, and that the walk kernel has one per layer (the window chains it walks: `walk[j]` for entry j).
struct TapEnt { size_t chain; int rank, px_begin, px_end, tile; };
struct TapEntries {
    std::vector<TapEnt> ents;
    std::vector<std::vector<size_t>> walk;
    size_t n_walk_wins = 0;
};

TapEntries tap_entries(const DaamCtx* c, const std::vector<TapChain>& chains, const TapKind& kind, int tile)
{
    TapEntries E;
    auto mine = [&](const TapChain& ch) { return ch.kind == kind && !ch.rides; };
    if (kind.is(TapRoute::Walk)) {
        // entry = the window chains of one layer, in recorded order.  An entry ends where its steps would pass the launch's step limit
        // (the pointer table in LDS holds the ENTRY's steps) or where a window's shape or strides differ from the entry's: the layer
        // then has another entry for its later windows -- never a window in two entries.
        std::vector<int> open(c->max_layers, -1), steps_in;
        for (size_t i = 0; i < chains.size(); ++i) {
            if (!mine(chains[i])) continue;
            const int layer = chains[i].slot % c->max_layers, n = (int)chains[i].steps.size();
            int e = open[layer];
            if (e < 0 || steps_in[e] + n > tap_mfma_max_steps() || !same_call_shape(chains[E.walk[e][0]].d(), chains[i].d())) {
                e = open[layer] = (int)E.walk.size();
                E.walk.emplace_back();
                steps_in.push_back(0);
            }
            E.walk[e].push_back(i);
            steps_in[e] += n;
            ++E.n_walk_wins;
        }
        for (auto& g : E.walk) E.ents.push_back({g[0], 0, 0, chains[g[0]].d().hw, tile});
        return E;
    }
    // slab kernel: the layers segment by segment (one cost per workgroup each): head_dim 160 first (few, light workgroups with the longest
    // step chains), 40 (the bulk), 80 (short chains), and last the TAIL of the head_dim-40 layers in half-size workgroups: 2.2 rounds of
    // indivisible 50-step chains leave a third of the chip idle for the last 100 us of the launch; half-length units empty it more evenly
    // (DAAM_SLAB_TAIL = percent of a head_dim-40 layer's pixels that go there; bit-identical sums either way).  Every XCD takes an eighth of
    // each segment.  Round 6 searched the order with a list-scheduling model (tools/slab_order_model.py) and measured its best candidate
    // ("columns": first halves heavy-first, second halves light-first, half-size units last) on the chip: 3 % SLOWER than this order for
    // every tail share (LABNOTES R6.2) -- a chain's speed depends on what shares its CU, which the model does not know.
    auto seg_rank = [](int d) { return d == 160 ? 0 : d == 40 ? 1 : 2; };
    for (size_t i = 0; i < chains.size(); ++i) {
        if (!mine(chains[i])) continue;
        const DaamQKDesc& d0 = chains[i].d();
        if (!kind.is(TapRoute::Slab)) { E.ents.push_back({i, 0, 0, d0.hw, tile}); continue; }
        const int r = seg_rank(d0.head_dim);
        const int tail_px = (r == 1 && d0.hw >= 64) ? (int)((int64_t)d0.hw * c->slab_tail_pct / 100 / 32) * 32 : 0;
        if (d0.hw - tail_px > 0) E.ents.push_back({i, r, 0, d0.hw - tail_px, tile});
        if (tail_px > 0) E.ents.push_back({i, 3, d0.hw - tail_px, d0.hw, tile / 2});
    }
    if (kind.is(TapRoute::Slab)) std::stable_sort(E.ents.begin(), E.ents.end(), [](const TapEnt& a, const TapEnt& b) { return a.rank < b.rank; });
    return E;
}

// Builds the tables of `kind` in the upload ring and enqueues their upload on `s`.  Ring region:
//   TapLayer[n] (Pair: the chain-A entries, then the chain-B entries, one per pair in the same order) | TapPtr[] | WalkWin[] | WalkEntry[]
// step pointers: the walk windows in entry order, else the chains in slot order (Pair: A's before its partner's).
int tap_tables(DaamCtx* c, const std::vector<TapChain>& chains, const TapKind& kind, int in_dtype, hipStream_t s, TapTables* out)
{
    const bool pair = kind.is(TapRoute::Pair), walk = kind.is(TapRoute::Walk), slab = kind.is(TapRoute::Slab);
    auto mine = [&](const TapChain& ch) { return ch.kind == kind && !ch.rides; };
    int tile = tap_tile_pixels(kind);
    bool w8 = false;
    if (kind.is(TapRoute::D64) && !c->no_w8) {
        // head_dim-64 launches with fp16 Q / K and fp16 sums: 256-pixel tiles on eight-wave workgroups (one K tile for twice the pixels)
        const int t8 = tap_d64_tile_pixels(in_dtype, c->acc_dtype, all_head_dim_64(chains, kind) ? 1 : 0);
        w8 = t8 != tile;
        tile = t8;
    }
    if (kind.is(TapRoute::Generic))                          // the generic kernel reads the sums first
        for (const TapChain& ch : chains)
            if (mine(ch)) {
                int rc = ensure_zeroed(c->layers[ch.slot], s);
                if (rc) return rc;
            }
    const TapEntries E = tap_entries(c, chains, kind, tile);
    const size_t n_layers = E.ents.size();
    size_t n_ptrs = 0;
    for (const TapChain& ch : chains)
        if (mine(ch)) n_ptrs += ch.steps.size() * (pair ? 2 : 1);
    const size_t bytes_layers = n_layers * (pair ? 2 : 1) * sizeof(TapLayer), bytes_tap = bytes_layers + n_ptrs * sizeof(TapPtr);
    const size_t bytes_wins = E.n_walk_wins * sizeof(WalkWin), bytes = bytes_tap + bytes_wins + E.walk.size() * sizeof(WalkEntry);
    size_t off = 0;
    hipError_t e = c->ring.alloc(bytes, &off);
    if (e != hipSuccess) return fail((int)e, "upload ring: %s", hipGetErrorString(e));
    TapLayer* hl = reinterpret_cast<TapLayer*>(c->ring.host + off);
    TapPtr* hp = reinterpret_cast<TapPtr*>(c->ring.host + off + bytes_layers);
    WalkWin* hw_wins = reinterpret_cast<WalkWin*>(c->ring.host + off + bytes_tap);
    WalkEntry* hw_ents = reinterpret_cast<WalkEntry*>(c->ring.host + off + bytes_tap + bytes_wins);
    *out = TapTables();
    int wg = 0, ptr = 0;
    std::vector<int> ptr_of(chains.size(), -1);                // a chain's step pointers are written once, both of its entries point at them
    auto put_ptrs = [&](size_t ci) {
        ptr_of[ci] = ptr;
        for (const Pending* p : chains[ci].steps) { hp[ptr].q = p->q; hp[ptr].k = p->k; ++ptr; }
    };
    for (size_t j = 0, win = 0; j < E.walk.size(); ++j) {      // (Walk) a window's step pointers follow the previous window's
        hw_ents[j].win_begin = (int32_t)win;
        hw_ents[j].n_win = (int32_t)E.walk[j].size();
        for (size_t i : E.walk[j]) {
            const Layer& wl = c->layers[chains[i].slot];
            hw_wins[win].acc = wl.acc;
            hw_wins[win].n_steps = (int32_t)chains[i].steps.size();
            hw_wins[win].fresh = wl.dirty ? 0 : 1;
            ++win;
            put_ptrs(i);
        }
    }
    for (size_t i = 0; i < chains.size() && !walk; ++i) {
        if (!mine(chains[i])) continue;
        put_ptrs(i);
        if (pair) put_ptrs((size_t)chains[i].partner);
    }
    int seg_begin[kMaxSlabSegs + 1] = {0}, n_seg = 0;
    int last_rank = -1;
    for (size_t j = 0; j < n_layers; ++j) {
        const TapEnt& en = E.ents[j];
        const TapChain& ch = chains[en.chain];
        fill_layer(c->layers[ch.slot], ch.d(), en.tile, &hl[j]);
        hl[j].wg_begin = wg;
        hl[j].n_steps = (int)ch.steps.size();
        if (walk) {                                          // the entry's steps: every window's
            hl[j].n_steps = 0;
            for (size_t i : E.walk[j]) hl[j].n_steps += (int)chains[i].steps.size();
        }
        hl[j].ptr_begin = ptr_of[en.chain];
        hl[j].px_begin = en.px_begin;
        hl[j].px_end = en.px_end;
        hl[j].tile_px = en.tile;
        hl[j].tiles_per_head = (en.px_end - en.px_begin + en.tile - 1) / en.tile;
        if (slab) {
            if (en.rank != last_rank) { seg_begin[n_seg++] = wg; last_rank = en.rank; }
            wg += hl[j].heads_kept / tap_slab_heads(ch.d().head_dim) * hl[j].tiles_per_head;   // tiles_per_head = tiles per slab
        } else {
            wg += hl[j].heads_kept * hl[j].tiles_per_head;
        }
        out->max_d = std::max(out->max_d, ch.d().head_dim);
        out->min_d = std::min(out->min_d, ch.d().head_dim);
        out->all_round = out->all_round && ch.d().round_logits;
        if (pair) {                                          // chain B: its own sums, fresh flag, K batch stride and pointer pair
            const TapChain& cb = chains[ch.partner];
            TapLayer& hb = hl[n_layers + j];
            fill_layer(c->layers[cb.slot], cb.d(), en.tile, &hb);
            hb.wg_begin = hl[j].wg_begin;
            hb.n_steps = hl[j].n_steps;
            hb.ptr_begin = ptr_of[ch.partner];
            hb.tiles_per_head = hl[j].tiles_per_head;
        }
    }
    seg_begin[n_seg] = wg;
    // daam_finalize_prepare: the output of the finalize that follows this launch is cleared by this (first) upload kernel
    const bool fold = c->fold_out && c->fold_stream == s;
    e = c->ring.commit(off, bytes, s, fold ? c->fold_out : nullptr, fold ? c->fold_bytes : 0);
    if (e != hipSuccess) return fail((int)e, "table upload: %s", hipGetErrorString(e));
    if (fold) {
        c->prep_out = c->fold_out;
        c->prep_stream = s;
        c->fold_out = nullptr;
    }
    out->kind = kind;
    out->in_dtype = in_dtype;
    out->w8 = w8;
    memset(&out->L, 0, sizeof out->L);
    out->L.layers = reinterpret_cast<const TapLayer*>(c->ring.dev + off);
    out->L.ptrs = reinterpret_cast<const TapPtr*>(c->ring.dev + off + bytes_layers);
    out->L.n_layers = (int)n_layers;
    out->L.tokens = c->tokens;
    out->L.total_wgs = wg;
    out->L.wgs_per_xcd = (wg + 7) / 8;
    out->L.n_seg = n_seg;
    for (int k = 0; k <= kMaxSlabSegs; ++k) out->L.seg_begin[k] = seg_begin[k];
    out->walk_wins = reinterpret_cast<const WalkWin*>(c->ring.dev + off + bytes_tap);
    out->walk_entries = reinterpret_cast<const WalkEntry*>(c->ring.dev + off + bytes_tap + bytes_wins);
    out->ring_begin = c->ring.cur_begin;
    out->ring_end = c->ring.cur_end;
    return 0;
}

// ---- stage 4 helper: the start gate's strike rule ---------------------------------------------------------------------------------
// start gate: the side kernels' workgroups count themselves in, the main kernel waits (one wave, bounded) until they are
// resident -- only for the kernels that carry the counter (the MFMA kinds).
// A gate that runs into its 200 us timeout means the side kernels were NOT running beside the caller's stream at that moment (one
// hardware queue, GPU_MAX_HW_QUEUES; or another process held the GPU): every gated flush then pays the 200 us for nothing.  The
// timeout counter is pinned host memory the gate kernels bump; the host reads it here WITHOUT synchronising, so it lags the
// enqueued flushes by however many are still in flight.  Rule (robust against that lag): since the gate was last armed, at least
// three timeouts AND at least half of the gated flushes enqueued so far timed out -> the gate rests for 64 flushes (said once),
// then is armed again with fresh counts.
void gate_count_strikes(DaamCtx* c)
{
    const unsigned now = *reinterpret_cast<volatile unsigned*>(c->gate_timeouts);
    if (c->gate_off_until && c->n_flushes >= c->gate_off_until) { c->gate_off_until = 0; c->gate_timeouts_seen = now; c->gate_enqueued = 0; }
    if (c->gate_off_until) return;
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

// record one validated call for `layer` (a layer, or a (window, layer) slot of a binned context)
int enqueue_slot(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d)
{
    if (!c->pending.empty() && c->pending.front().d.in_dtype != d->in_dtype)
        return fail(DAAM_E_STATE, "mixed activation dtypes in one deferred batch: flush first");
    if (c->pending_count.size() != c->layers.size()) {
        c->pending_count.assign(c->layers.size(), 0);
        c->pending_last.assign(c->layers.size(), -1);
    }
    if (c->pending_count[layer] > 0) {
        // every recorded step of a layer must share shape and strides (hw among them, which check_qk ties to the layer anyway)
        if (!same_call_shape(c->pending[c->pending_last[layer]].d, *d))
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

}  // namespace

int check_qk(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d)
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

extern "C" {

int daam_tap_qk(DaamCtx* c, int layer, const void* q, const void* k, const DaamQKDesc* d, void* stream)
{
    int rc = check_qk(c, layer, q, k, d);
    if (rc) return rc;
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "immediate tap with deferred taps pending: flush first");
    DeviceGuard on_device(c);
    const int slot = c->slot_of(layer);                        // the window of this step (= layer without windows)
    const TapKind kind = use_mfma(c, *d, q, k) ? mfma_kind(c, *d, q, k) : TapKind{};
    if (kind.is(TapRoute::Generic) && (rc = ensure_zeroed(c->layers[slot], (hipStream_t)stream))) return rc;
    TapTables t;
    t.kind = kind;
    t.in_dtype = d->in_dtype;
    t.min_d = t.max_d = d->head_dim;
    t.all_round = d->round_logits;
    TapLaunch& L = t.L;
    memset(&L, 0, sizeof L);
    fill_layer(c->layers[slot], *d, tap_tile_pixels(kind), &L.one);
    L.one_ptr.q = q;
    L.one_ptr.k = k;
    L.n_layers = 1;
    L.tokens = c->tokens;
    L.total_wgs = L.one.heads_kept * L.one.tiles_per_head;
    L.wgs_per_xcd = (L.total_wgs + 7) / 8;
    c->last_block[0] = 256;
    hipError_t e = tap_launch_kind(c, t, (hipStream_t)stream, &c->last_grid[0], &c->last_lds[0]);
    if (e != hipSuccess) return fail((int)e, "tap launch: %s", hipGetErrorString(e));
    c->last_kernels[0] = tap_kernel_name(kind);
    c->layers[slot].dirty = true;
    c->layers[slot].zero_pending = false;
    ++c->tap_steps[layer];
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
    std::vector<TapChain> chains = tap_group(c);
    tap_route(c, chains, in_dtype);
    std::vector<TapKind> kinds;                              // first-seen order
    for (const TapChain& ch : chains)
        if (!ch.rides && std::find(kinds.begin(), kinds.end(), ch.kind) == kinds.end()) kinds.push_back(ch.kind);
    // pass 1: the tables of every kernel kind -> ring -> device (all on the caller's stream)
    int rc = 0;
    std::vector<TapTables> prepared;
    for (const TapKind& kind : kinds) {
        TapTables t;
        if ((rc = tap_tables(c, chains, kind, in_dtype, s, &t))) break;
        prepared.push_back(t);
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
    if (forked && c->gate_timeouts) gate_count_strikes(c);
    bool gate = forked && !c->no_start_gate && !c->gate_off_until && c->d_started;
    for (size_t i = 0; i < prepared.size(); ++i)
        if (i != main_idx && prepared[i].kind.is(TapRoute::Generic)) gate = false;
    unsigned gate_wgs = 0;
    int n_side = 0, grid_total = 0;
    std::string launched_names;
    for (size_t pi : launch_order) {
        if (rc) break;
        TapTables& pr = prepared[pi];
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
        hipError_t e = tap_launch_kind(c, pr, ks, &grid, &c->last_lds[0]);
        grid_total += grid;
        if (e != hipSuccess) { rc = fail((int)e, "tap launch: %s", hipGetErrorString(e)); break; }
        launched_names += (launched_names.empty() ? "" : "+") + std::string(tap_kernel_name(pr.kind));
        e = c->ring.release_range(pr.ring_begin, pr.ring_end, ks);
        if (e != hipSuccess) { rc = fail((int)e, "event record: %s", hipGetErrorString(e)); break; }
        if (ks != s) {
            if (hipEventRecord(c->aux_join[n_side], ks) != hipSuccess) { rc = fail(DAAM_E_STATE, "stream join failed"); break; }
            ++n_side;
        }
        for (const TapChain& ch : chains)                      // (a pair's partner carries its chain A's kind)
            if (ch.kind == pr.kind) { c->layers[ch.slot].dirty = true; c->layers[ch.slot].zero_pending = false; }
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
    for (const TapTables& pr : prepared)
        if (pr.block512()) c->last_block[0] = 512;
    c->last_kernels[0] = launched_names;
    c->last_flush_kernels = (int)launch_order.size();
    c->last_flush_side = n_side;
    c->last_flush_steps = 0;
    for (const TapChain& ch : chains) c->last_flush_steps = std::max(c->last_flush_steps, (int)ch.steps.size());
    ++c->n_flushes;
    c->drop_pending();
    c->fold_out = nullptr;                                     // one-shot: never carried to a later launch
    return rc;
}

}  // extern "C"
