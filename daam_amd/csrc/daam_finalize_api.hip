// Finalize half of the host API (include/daam_hip.h): daam_finalize_prepare, daam_finalize, daam_finalize_groups and
// daam_finalize_bins.  One plan (fin_plan: which keys, in which class, of which group, the chunking of the pipelined x2 kernel
// and the device tables), one way to get tables to the device (FinTables), one launcher (fin_launch_classes).  Two families of
// class kernels sit on top: the single-prompt ones (fin_single) and the *_grouped_kernel forms (fin_grouped).
#include "daam_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kFinClasses = 5;       // 0 = same size (clamp + mean), 1 = x2 (32 -> 64), 2 = x4 (16 -> 64), 3 = general kernel, 4 = x0.5 (128 -> 64)
constexpr int kFinPipe = kFinClasses;   // fin_chunks: the x2 class on the software-pipelined kernel

// The selected keys of a call, class by class and inside a class group by group (stable: layer-major order inside a group; a
// group's keys are contiguous in the FinKey array and in the pointer tables of the pipelined x2 kernel, so no chunk straddles two
// groups).  A single-prompt call is the one-group case.
struct FinPlan {
    int n_groups = 1, total = 0, max_side = 0;
    int max_rows = 0, sum_rows = 0;
    int n[kFinClasses] = {0, 0, 0, 0, 0};        // keys of the class
    int max_n[kFinClasses] = {0, 0, 0, 0, 0};    // ... of its largest group
    int first[kFinClasses] = {0, 0, 0, 0, 0};    // index of its first key in the FinKey array
    bool have[kFinClasses] = {false, false, false, false, false};   // the class has keys and a kernel of its own
    int begin[kFinClasses][kFinMaxGroups], count[kFinClasses][kFinMaxGroups];   // a group's keys inside the class
    int n_of[kFinMaxGroups];                     // keys of the group over every class
    bool mfma_up = false, pipe_up = false, fold_same = false;
    int pipe_chunks = 0, pipe_per = 0, pipe_nk = 0, pipe_stride = 0, same_per = 0;
    size_t key_bytes = 0, ptr_bytes = 0;
    size_t ptr_per_group = 0, same_per_group = 0;   // entries of a group in the two pointer tables
    std::vector<char> tab;           // FinKey array (class order) | pointer table of the pipelined x2 kernel | folded same-size pointers
    const FinKey* keys(int cls) const { return reinterpret_cast<const FinKey*>(tab.data()) + first[cls]; }
};

int fin_env(const char* name)
{
    const char* v = getenv(name);
    return v ? atoi(v) : 0;
}

// Chunk count of a class kernel over `n` keys (of the largest group) and `rows` token rows (of every group).
int fin_chunks(int cls, int n, int rows)
{
    static const int env_chunks = fin_env("DAAM_FIN_CHUNKS");
    static const int env_pipe_chunks = fin_env("DAAM_FIN_PIPE_CHUNKS");   // pipelined x2 kernel only (A/B)
    static const int env_up_chunks = fin_env("DAAM_FIN_UP_CHUNKS");       // LDS up kernels only (A/B)
    // 154 workgroups per chunk: 4 chunks for the 100 same-size keys of SDXL-1024, up to 9 (1386 workgroups) for the 1000 of
    // SDXL-2048.  Round 2 had 16 there; round 4's sweep (tools/exp/fin_chunks_sweep.sh: 4 ... 64 chunks) has its optimum at
    // 8 - 10 -- the x0.5 class now streams beside this one on a side stream, and every chunk ends in 315 k atomics per
    // token plane: 0.186 -> 0.159 ms for the SDXL-2048 call (0.59 -> 0.69 of the HBM peak)
    if (cls == 0) return std::max(1, std::min(n, env_chunks ? env_chunks : std::min(9, std::max(4, n / 32))));
    if (cls == 3) return std::max(1, std::min(n, 32));
    // x2 class chunking: ~1000 workgroups (one full round at 4 workgroups per CU) measured best -- fewer leaves a ragged
    // tail, more pays the per-workgroup reduction + atomics too often
    const int env = cls == kFinPipe ? env_pipe_chunks : env_up_chunks;
    const int want = env ? env : env_chunks ? env_chunks : std::max(1, (1024 + rows / 2) / rows);
    if (cls == kFinPipe) return std::max(1, std::min(want, (n + 7) / 8));
    // each wave takes keys first, first + 4*n_chunks, ...: at most 64 per wave (4 key lanes per workgroup; the MFMA kernel of
    // class 1 has 2 and is chunked per launch).  Few keys: at least 4 per wave -- a workgroup ends in a four-wave LDS reduction
    // + 4096 atomics, which one key per wave does not pay for: SD-v1.5's 48 x4 keys in 3 chunks instead of 12 take 10 us less
    return std::max(std::max(1, std::min((n + 15) / 16, want)), (n + 127) / 128);
}

// token rows a finalize call covers (ABI v6: the caller may pass the prompt's n_tokens + 2, daam/trace.py:127)
int fin_rows(const DaamCtx* c, int n_rows) { return (n_rows <= 0 || n_rows > c->tokens) ? c->tokens : n_rows; }

// The plan over `n_layers` entries of `layers` whose planes are of `dtype`: the context's sums (c->layers / max_layers /
// acc_dtype), the window slots of a binned context, or f32 scratch planes (daam_finalize_bins).  Key i of that table (layer-major,
// heads inside) belongs to group key_group[i] (< 0: not selected), rows[g] token rows each; without key_group there is one group,
// the keys key_mask selects (NULL: all).
int fin_plan(DaamCtx* c, const Layer* layers, int n_layers, int dtype, const uint8_t* key_mask, const int32_t* key_group, int n_groups,
             const int* rows, FinPlan& P)
{
    struct Sel { FinKey k; int cls, g; };
    std::vector<Sel> sel;
    P.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g) {
        for (int cls = 0; cls < kFinClasses; ++cls) P.count[cls][g] = 0;
        P.n_of[g] = 0;
        P.max_rows = std::max(P.max_rows, rows[g]);
        P.sum_rows += rows[g];
    }
    int pos = 0, up32_tab = -1;
    for (int i = 0; i < n_layers; ++i) {
        const Layer& l = layers[i];
        if (!l.configured) continue;
        int cls = 3;
        if (!c->force_generic) {
            if (l.tab < 0 && (l.hw % 8) == 0) cls = 0;
            else if (l.tab >= 0 && finalize_up_supported(l.side, c->out_side)) cls = l.side == 32 ? 1 : 2;
            else if (l.tab >= 0 && finalize_down2_supported(l.side, c->out_side)) cls = 4;
        }
        for (int h = 0; h < l.heads; ++h, ++pos) {
            const int g = key_group ? key_group[pos] : (key_mask && !key_mask[pos]) ? -1 : 0;
            if (g < 0) continue;
            Sel s;
            s.k.base = static_cast<const char*>(l.acc) + (size_t)h * c->tokens * l.hw * acc_elem(dtype);
            s.k.side = l.side;
            s.k.tab = l.tab;
            s.cls = cls;
            s.g = g;
            sel.push_back(s);
            if (cls == 3 && l.tab >= 0) P.max_side = std::max(P.max_side, l.side);
            if (cls == 1) up32_tab = l.tab;                    // (one table per side: the same for every x2 key)
            ++P.count[cls][g];
            ++P.n_of[g];
            ++P.total;
        }
    }
    if (P.total == 0) return fail(DAAM_E_NOMAPS, "no heat maps selected");
    if (P.max_side > 128) return fail(DAAM_E_UNSUPPORTED, "map side %d > 128 not supported by finalize", P.max_side);
    int next[kFinClasses][kFinMaxGroups];                      // where the next key of (class, group) goes
    for (int cls = 0, at = 0; cls < kFinClasses; ++cls) {
        P.first[cls] = at;
        for (int g = 0; g < n_groups; ++g) {
            next[cls][g] = at;
            P.begin[cls][g] = P.count[cls][g] ? at - P.first[cls] : 0;   // (a kernel reads keys[0].tab: stay inside the class)
            P.max_n[cls] = std::max(P.max_n[cls], P.count[cls][g]);
            at += P.count[cls][g];
        }
        P.n[cls] = at - P.first[cls];
    }
    // x2 class on the matrix cores (fp16 planes, fp16-exact tap matrix)?
    P.mfma_up = P.n[1] && up32_tab == c->up32_tab && c->d_up32_ops && c->tab_fp16_exact[up32_tab] && !c->no_mfma_finalize;
    // ... on the software-pipelined kernel (daam_finalize_pipe.hip): workgroup = (token, key chunk), every wave walks ALL keys
    // of its chunk from a pointer table padded with the all-zero plane to one even length >= 4 (+ what the ring prefetches
    // past the end).  ~1000 workgroups of 2 waves = one resident round at 2 waves per SIMD, over the whole launch (every group's
    // rows); one chunk length for every group.
    P.pipe_up = P.mfma_up && !c->no_pipe_finalize && c->d_zero_planes;
    // bf16 / f32 sums (round 6): the pipelined kernel only (bf16: the tap matrix must split into two bf16 MFMA operands); the round-2 MFMA
    // kernels behind DAAM_NO_PIPE_FINALIZE take fp16 planes
    if (dtype == DAAM_BF16) P.pipe_up = P.pipe_up && c->d_up32_ops_bf16;
    if (dtype != DAAM_F16) P.mfma_up = P.pipe_up;
    if (P.pipe_up) {
        P.pipe_chunks = fin_chunks(kFinPipe, P.max_n[1], P.sum_rows);
        P.pipe_per = (P.max_n[1] + P.pipe_chunks - 1) / P.pipe_chunks;
        P.pipe_nk = std::max(4, (P.pipe_per + 1) & ~1);
        P.pipe_stride = (P.pipe_nk + finalize_pipe_ring(dtype) + 2) & ~1;
    }
    // The same-size (64 x 64) keys ride along in the pipelined kernel (every wave adds its share of them to its accumulators
    // before the x2 loop) unless they outnumber the x2 keys 2 : 1 -- then they keep their own streaming kernel.
    P.fold_same = P.pipe_up && P.n[0] && c->out_side == 64 && P.n[0] <= 2 * P.n[1] && !c->no_fold_same;
    P.same_per = P.fold_same ? (P.max_n[0] + P.pipe_chunks - 1) / P.pipe_chunks : 0;
    for (int cls = 0; cls < kFinClasses; ++cls) P.have[cls] = P.n[cls] && !(cls == 0 && P.fold_same);
    P.key_bytes = ((size_t)P.total * sizeof(FinKey) + 63) & ~size_t(63);
    P.ptr_per_group = (size_t)P.pipe_chunks * P.pipe_stride;
    P.same_per_group = (size_t)P.pipe_chunks * P.same_per;
    P.ptr_bytes = P.ptr_per_group * n_groups * sizeof(unsigned long long);
    P.tab.assign(P.key_bytes + P.ptr_bytes + P.same_per_group * n_groups * sizeof(unsigned long long), 0);
    FinKey* keys = reinterpret_cast<FinKey*>(P.tab.data());
    for (const Sel& s : sel) keys[next[s.cls][s.g]++] = s.k;
    if (P.pipe_up) {
        unsigned long long* pt = reinterpret_cast<unsigned long long*>(P.tab.data() + P.key_bytes);
        unsigned long long* st = pt + P.ptr_per_group * n_groups;
        const unsigned long long zero = reinterpret_cast<unsigned long long>(c->d_zero_planes);
        for (int g = 0; g < n_groups; ++g) {
            const FinKey* k1 = P.keys(1) + P.begin[1][g];
            const FinKey* k0 = P.keys(0) + P.begin[0][g];
            for (int ch = 0; ch < P.pipe_chunks; ++ch) {
                for (int j = 0; j < P.pipe_stride; ++j) {
                    const int k = ch * P.pipe_per + j;
                    pt[g * P.ptr_per_group + (size_t)ch * P.pipe_stride + j] =
                        (j < P.pipe_per && k < P.count[1][g]) ? reinterpret_cast<unsigned long long>(k1[k].base) : zero;
                }
                for (int j = 0; j < P.same_per; ++j) {
                    const int k = ch * P.same_per + j;
                    st[g * P.same_per_group + (size_t)ch * P.same_per + j] =
                        k < P.count[0][g] ? reinterpret_cast<unsigned long long>(k0[k].base) : 0ull;
                }
            }
        }
    }
    return 0;
}

// a zeroing still owed to a layer since daam_reset comes before anything reads its sums
int fin_zero_owed(Layer* layers, size_t n_layers, hipStream_t s)
{
    for (size_t i = 0; i < n_layers; ++i)
        if (layers[i].configured) {
            int zrc = ensure_zeroed(layers[i], s);
            if (zrc) return zrc;
        }
    return 0;
}

// The tables of a call on the device, for the kernels enqueued on `s` while this object lives.  Tables that may be cached
// (the plan's; a generation's compute_global_heat_map() selects the same keys at the same addresses as the previous one) stay
// in d_fin_tab between calls: the same bytes on the same stream are not uploaded again, other bytes replace them -- unless
// kernels enqueued on ANOTHER stream may still be reading them.  Everything else sits in a ring region, which the destructor
// hands back behind whatever was launched.
struct FinTables {
    DaamCtx* c;
    hipStream_t s;
    const char* dev = nullptr;
    bool ring_held = false;
    size_t ring_begin = 0, ring_end = 0;
    FinTables(DaamCtx* ctx, hipStream_t stream) : c(ctx), s(stream) {}
    ~FinTables() { release(); }
    FinTables(const FinTables&) = delete;
    FinTables& operator=(const FinTables&) = delete;
    void release() { if (ring_held) (void)c->ring.release_range(ring_begin, ring_end, s); ring_held = false; }

    bool hit(const std::vector<char>& tab) const {
        return !c->no_fin_cache && c->fin_tab_valid && c->fin_tab_stream == s && tab.size() == c->fin_tab_host.size() &&
               memcmp(tab.data(), c->fin_tab_host.data(), tab.size()) == 0;
    }
    bool cacheable(const std::vector<char>& tab) const {
        return !c->no_fin_cache && c->d_fin_tab && tab.size() <= DaamCtx::kFinTabCap && (!c->fin_tab_valid || c->fin_tab_stream == s);
    }
    // bytes -> pinned ring -> `dst` (NULL: the region's device twin, held) by the upload kernel, which also clears `zero`
    int upload(const void* bytes, size_t n, char* dst, void* zero, size_t zero_bytes) {
        size_t off = 0;
        HIP_TRY(c->ring.alloc(n, &off));
        memcpy(c->ring.host + off, bytes, n);
        ring_begin = c->ring.cur_begin;
        ring_end = c->ring.cur_end;
        ring_held = true;
        dev = dst ? dst : c->ring.dev + off;
        hipError_t e = launch_upload(const_cast<char*>(dev), c->ring.host_dev + off, n, zero, zero_bytes, s);
        if (dst || e != hipSuccess) release();                 // a staging region is free once the upload kernel has run
        if (e != hipSuccess) return fail((int)e, "table upload: %s", hipGetErrorString(e));
        return 0;
    }
    // the plan's tables (is_hit: hit(tab)); `zero` (optional) is cleared in the same launch
    int put(const std::vector<char>& tab, bool is_hit, void* zero, size_t zero_bytes) {
        if (is_hit) {
            dev = c->d_fin_tab;
            if (!zero) return 0;
            hipError_t e = launch_upload(nullptr, nullptr, 0, zero, zero_bytes, s);
            return e == hipSuccess ? 0 : fail((int)e, "output zeroing: %s", hipGetErrorString(e));
        }
        if (!cacheable(tab)) return upload(tab.data(), tab.size(), nullptr, zero, zero_bytes);
        c->fin_tab_valid = false;
        int rc = upload(tab.data(), tab.size(), c->d_fin_tab, zero, zero_bytes);
        if (rc) return rc;
        c->fin_tab_host = tab;
        c->fin_tab_valid = true;
        c->fin_tab_stream = s;
        return 0;
    }
};

bool fin_out_zeroable(const DaamCtx* c, const float* out, int rows)
{
    const size_t out_bytes = sizeof(float) * rows * (size_t)c->out_h * c->out_w;
    return out_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
}

// What the class kernels of both families share of their launch descriptors (per launch: the largest group's key count and
// rows; a single-prompt call adds its 1/N, a grouped one its FinGroup table).
FinLaunch fin_class_launch(const DaamCtx* c, const FinPlan& P, int cls, const char* tab_dev, float* out)
{
    FinLaunch L;
    memset(&L, 0, sizeof L);
    L.keys = reinterpret_cast<const FinKey*>(tab_dev) + P.first[cls];
    L.tab_idx = c->d_tab_idx;
    L.tab_w = c->d_tab_w;
    L.out = out;
    L.n_keys = P.max_n[cls];
    L.n_chunks = fin_chunks(cls, P.max_n[cls], P.sum_rows);
    L.tokens = P.max_rows;                                     // grid dimension / bound of every class kernel; a key's planes keep their [tokens] stride
    L.out_side = c->out_side;
    L.max_side = P.max_side;
    return L;
}

FinPipeLaunch fin_pipe_launch(const DaamCtx* c, const FinPlan& P, int dtype, const char* tab_dev, float* out)
{
    FinPipeLaunch PL;
    memset(&PL, 0, sizeof PL);
    PL.key_ptrs = reinterpret_cast<const unsigned long long*>(tab_dev + P.key_bytes);
    PL.same_ptrs = P.fold_same ? reinterpret_cast<const unsigned long long*>(tab_dev + P.key_bytes + P.ptr_bytes) : nullptr;
    PL.same_per = P.same_per;
    PL.mfma_ops = dtype == DAAM_BF16 ? c->d_up32_ops_bf16 : c->d_up32_ops;
    PL.out = out;
    PL.n_chunks = P.pipe_chunks;
    PL.nk_pad = P.pipe_nk;
    PL.ptr_stride = P.pipe_stride;
    PL.tokens = P.max_rows;
    return PL;
}

std::string fin_name(const char* kernel, const std::string& what) { return std::string(kernel) + "<" + what + ">"; }

// The class kernels that need nothing but their descriptor: what daam_last_kernels calls them -- stem + "_kernel" or
// "_grouped_kernel" + targ + "<dtype>" -- and the launcher of both forms (daam_finalize.h).  The x2 class has three more kernels
// (pipelined, round-2 MFMA, paired with the same-size class), which fin_single / fin_grouped pick ahead of this table.
const struct FinClass {
    const char* stem;
    const char* targ;
    FinClassLauncher* launch;
} kFinClass[kFinClasses] = {
    {"finalize_same", "", launch_finalize_same},
    {"finalize_up", "<32>", launch_finalize_up<32>},
    {"finalize_up", "<16>", launch_finalize_up<16>},
    {"finalize", "", launch_finalize},
    {"finalize_down2", "", launch_finalize_down2},
};
hipError_t fin_launch_class(int cls, const FinLaunch& L, const FinGroupLaunch* G, int n_groups, int dtype, hipStream_t s, int* grid,
                            int* lds, std::string* name)
{
    const FinClass& k = kFinClass[cls];
    *name = std::string(k.stem) + (G ? "_grouped_kernel" : "_kernel") + k.targ + "<" + dtype_name(dtype) + ">";
    return k.launch(L, G, n_groups, dtype, s, grid, lds);
}

// Launches the kernel of every class in P.have: launch_class(cls, stream, &grid, &lds, &name) enqueues it and names it.
// Several classes: the issue-bound x2 kernel keeps the caller's stream; every other class (HBM streams with few registers:
// their waves fit beside the two heavy waves of a SIMD) goes to an auxiliary stream forked from / joined to the caller's by
// events, launched FIRST -- SDXL-1024: 63 MB of same-size planes stream under 158 MB of x2 planes; SD-v1.5: three classes side
// by side instead of three serial launches.  Records what daam_last_launch / daam_last_kernels report (`prefix` first) and
// closes the profiled span.
template <typename LaunchClass>
int fin_launch_classes(DaamCtx* c, const FinPlan& P, int dtype, hipStream_t s, const char* what, std::string prefix,
                       LaunchClass launch_class)
{
    // (an event fork / join costs ~15 us of queue latency per finalize call: only worth it for a side class of tens of MB --
    // SD-v1.5's 1.6 MB x4 class runs 10 us faster serially behind the pipelined kernel)
    int n_classes = 0;
    size_t side_bytes = 0;
    for (int cls = 0; cls < kFinClasses; ++cls) {
        if (!P.have[cls]) continue;
        ++n_classes;
        if (cls == 1) continue;
        for (int k = 0; k < P.n[cls]; ++k) side_bytes += (size_t)c->tokens * P.keys(cls)[k].side * P.keys(cls)[k].side * acc_elem(dtype);
    }
    bool fork = P.pipe_up && n_classes > 1 && n_classes <= DaamCtx::kAux + 1 && !c->no_side_stream && side_bytes >= ((size_t)16 << 20);
    if (fork) {
        hipError_t ae = ensure_aux(c);
        if (ae != hipSuccess || hipEventRecord(c->aux_fork, s) != hipSuccess) fork = false;    // serial launches still correct
    }
    c->last_block[1] = 256;
    c->last_grid[1] = 0;
    c->last_lds[1] = 0;
    int n_side = 0;
    const int order[kFinClasses] = {0, 2, 3, 4, 1};            // the x2 class last: side kernels are resident when it fills the chip
    for (int oi = 0; oi < kFinClasses; ++oi) {
        const int cls = order[oi];
        if (!P.have[cls]) continue;
        hipStream_t ks = s;
        if (fork && cls != 1) {
            ks = c->aux_stream[n_side];
            if (hipStreamWaitEvent(ks, c->aux_fork, 0) != hipSuccess) ks = s;
        }
        int grid = 0, lds = 0;
        std::string name;
        hipError_t e = launch_class(cls, ks, &grid, &lds, &name);
        if (e == hipSuccess && ks != s) {
            e = hipEventRecord(c->aux_join[n_side], ks);
            ++n_side;
        }
        if (e != hipSuccess) {
            for (int i = 0; i < n_side; ++i) (void)hipStreamWaitEvent(s, c->aux_join[i], 0);
            return fail((int)e, "%s launch (class %d): %s", what, cls, hipGetErrorString(e));
        }
        prefix += (prefix.empty() ? "" : "+") + name;
        c->last_grid[1] += grid;
        c->last_lds[1] = std::max(c->last_lds[1], lds);
    }
    bool joined = true;
    for (int i = 0; i < n_side; ++i) joined = (hipStreamWaitEvent(s, c->aux_join[i], 0) == hipSuccess) && joined;
    if (!joined) return fail(DAAM_E_STATE, "stream join failed");
    c->last_fin_side = n_side;
    c->last_kernels[1] = prefix;
    if (c->profile) { (void)hipEventRecord(c->prof_event(1, 1), s); ++c->hist_count[1]; }
    return 0;
}

// ---- outputs or layers of unequal sides: finalize_rect_kernel (daam_finalize_rect.hip) --------------------------------------------
// Every selected key of such a context takes the one kernel, whatever its own shape: one launch for a single map
// (finalize_rect_kernel) or for N groups (finalize_rect_grouped_kernel, grid z = group).  The key table goes through the device
// table cache like the square plan's; the output is cleared by the table-upload launch (single map) or by zero_groups_kernel.
// key_mask / key_group / rows as fin_plan.
int fin_rect(DaamCtx* c, Layer* layers, int n_layers, int dtype, const uint8_t* key_mask, const int32_t* key_group, int n_groups,
             const int* rows, float* out, size_t group_stride, hipStream_t s)
{
    std::vector<std::vector<FinRectKey>> per_group(n_groups);
    int plane_cap = 0, tmp_cap = 0, pos = 0, total = 0;
    for (int i = 0; i < n_layers; ++i) {
        Layer& l = layers[i];
        if (!l.configured) continue;
        // Layers get their table pair when they are configured; only a square layer configured before the context turned
        // rectangular (output sides equal, a later layer's not) is still without one.  rect_tab then allocates and copies with
        // the blocking calls, once per such (h, w): the first finalize of that context synchronises with the device here.
        int rc = rect_tab(c, l);
        if (rc) return rc;
        for (int h = 0; h < l.heads; ++h, ++pos) {
            const int g = key_group ? key_group[pos] : (key_mask && !key_mask[pos]) ? -1 : 0;
            if (g < 0) continue;
            FinRectKey k;
            k.base = static_cast<const char*>(l.acc) + (size_t)h * c->tokens * l.hw * acc_elem(dtype);
            k.h = (int16_t)l.h;
            k.w = (int16_t)l.w;
            k.tab = l.rtab;
            per_group[g].push_back(k);
            ++total;
            if (l.rtab >= 0) {
                plane_cap = std::max(plane_cap, (l.hw + 3) & ~3);
                tmp_cap = std::max(tmp_cap, l.h * c->out_w);
            }
        }
    }
    if (total == 0) return fail(DAAM_E_NOMAPS, "no heat maps selected");
    const size_t lds = fin_rect_lds_bytes(c->out_h, c->out_w, plane_cap, tmp_cap);
    if (lds > kFinRectMaxLds)
        return fail(DAAM_E_UNSUPPORTED, "finalize of %d x %d maps from these planes needs %zu bytes of LDS per workgroup (limit %zu)",
                    c->out_h, c->out_w, lds, kFinRectMaxLds);
    std::vector<char> tab(((size_t)total * sizeof(FinRectKey) + 63) & ~size_t(63), 0);
    FinRectKey* keys = reinterpret_cast<FinRectKey*>(tab.data());
    int begin[kFinMaxGroups], max_n = 0, max_rows = 0, sum_rows = 0;
    for (int g = 0, at = 0; g < n_groups; ++g) {
        begin[g] = at;
        for (const FinRectKey& k : per_group[g]) keys[at++] = k;
        max_n = std::max(max_n, (int)per_group[g].size());
        max_rows = std::max(max_rows, rows[g]);
        sum_rows += rows[g];
    }
    const size_t plane = (size_t)c->out_h * c->out_w;
    const bool single = n_groups == 1;
    const size_t out_bytes = sizeof(float) * rows[0] * plane;
    const bool zero_in_upload = single && fin_out_zeroable(c, out, rows[0]);
    if (single && !zero_in_upload) {
        hipError_t ze = hipMemsetAsync(out, 0, out_bytes, s);
        if (ze != hipSuccess) return fail((int)ze, "output memset: %s", hipGetErrorString(ze));
    }
    if (c->profile) (void)hipEventRecord(c->prof_event(1, 0), s);
    FinTables T(c, s);
    int rc = T.put(tab, T.hit(tab), zero_in_upload ? out : nullptr, zero_in_upload ? out_bytes : 0);
    if (rc) return rc;
    if (!single) {
        hipError_t ze = launch_zero_groups(out, group_stride, (int)plane, rows, n_groups, s);
        if (ze != hipSuccess) return fail((int)ze, "output zeroing: %s", hipGetErrorString(ze));
    }
    FinRectGroupLaunch G;
    memset(&G, 0, sizeof G);
    FinRectLaunch& L = G.L;
    L.keys = reinterpret_cast<const FinRectKey*>(T.dev);
    L.tab_idx = c->d_rtab_idx;
    L.tab_w = c->d_rtab_w;
    L.out = out;
    L.n_keys = max_n;
    // token rows x key chunks, aimed at 1024 workgroups = four per CU on 256 CUs.  By arithmetic, not by measurement: the
    // 160 KB of a CU's LDS hold two to five of the tiles the tested shapes need; no other chunk count has been timed.
    L.n_chunks = std::max(1, std::min(max_n, (1024 + sum_rows / 2) / sum_rows));
    L.tokens = max_rows;
    L.out_h = c->out_h;
    L.out_w = c->out_w;
    L.plane_cap = plane_cap;
    for (int g = 0; g < n_groups; ++g) {
        G.g[g].key_begin = begin[g];
        G.g[g].n_keys = (int)per_group[g].size();
        G.g[g].rows = rows[g];
        G.g[g].inv_n = 1.0f / (float)per_group[g].size();
        G.g[g].out_off = (int64_t)((size_t)g * group_stride);
    }
    int grid = 0, lds_used = 0;
    if (single) L.inv_n = G.g[0].inv_n;
    const hipError_t e = launch_finalize_rect(L, single ? nullptr : &G, n_groups, tmp_cap, dtype, s, &grid, &lds_used);
    if (e != hipSuccess) return fail((int)e, "rectangular finalize launch: %s", hipGetErrorString(e));
    c->last_block[1] = 256;
    c->last_grid[1] = grid;
    c->last_lds[1] = lds_used;
    c->last_fin_side = 0;
    c->last_kernels[1] = fin_name(single ? "finalize_rect_kernel" : "finalize_rect_grouped_kernel", dtype_name(dtype));
    if (c->profile) { (void)hipEventRecord(c->prof_event(1, 1), s); ++c->hist_count[1]; }
    return 0;
}

// Key ranges of the chunks of the x2 MFMA finalize: equal shares (even boundaries; the two key lanes of a workgroup take the
// keys of its range alternately).  Shares shrinking with the dispatch round of a chunk's workgroups (the SIMD arbitrates by
// age: the first 256 workgroups finish their loop in 23 us, the last 256 in 40 us) were tried and changed nothing -- the kernel
// is throughput-bound from its first to its last microsecond, the age order only decides who waits.
void finalize_chunk_ranges(int n_keys, int n_chunks, FinLaunch* L)
{
    const int pairs = (n_keys + 1) / 2;
    for (int c = 0; c <= n_chunks; ++c)
        L->chunk_begin[c] = (int16_t)std::min(n_keys, 2 * (int)(((int64_t)pairs * c + n_chunks - 1) / n_chunks));
    L->chunk_begin[n_chunks] = (int16_t)n_keys;
}

// One global heat map on the single-prompt class kernels, over the context's own sums: the keys key_mask selects, or those of
// group 0 of key_group.
int fin_single(DaamCtx* c, const uint8_t* key_mask, const int32_t* key_group, int n_rows, float* out, hipStream_t s)
{
    const int rows = fin_rows(c, n_rows);
    // zeroed ahead of this call (daam_finalize_prepare, same buffer, same rows, same stream)?  One-shot.
    const bool prepared = c->prep_out == out && c->prep_stream == s && c->prep_rows == rows;
    c->prep_out = c->fold_out = nullptr;
    int rc = fin_zero_owed(c->layers.data(), c->layers.size(), s);
    if (rc) return rc;
    const int dtype = c->acc_dtype;
    if (c->rect()) return fin_rect(c, c->layers.data(), c->max_layers, dtype, key_mask, key_group, 1, &rows, out, 0, s);
    FinPlan P;
    if ((rc = fin_plan(c, c->layers.data(), c->max_layers, dtype, key_mask, key_group, 1, &rows, P))) return rc;
    const size_t out_bytes = sizeof(float) * rows * (size_t)c->out_side * c->out_side;
    // the output is accumulated with atomics: it is zeroed by the table-upload launch unless daam_finalize_prepare had it done
    const bool zero_in_upload = fin_out_zeroable(c, out, rows);
    if (!zero_in_upload && !prepared) {
        hipError_t ze = hipMemsetAsync(out, 0, out_bytes, s);
        if (ze != hipSuccess) return fail((int)ze, "output memset: %s", hipGetErrorString(ze));
    }
    if (c->profile) (void)hipEventRecord(c->prof_event(1, 0), s);    // timed: what this call launches (table upload + zeroing if needed, class kernels)
    void* zero_ptr = (zero_in_upload && !prepared) ? out : nullptr;
    FinTables T(c, s);
    if ((rc = T.put(P.tab, T.hit(P.tab), zero_ptr, zero_ptr ? out_bytes : 0))) return rc;
    const float inv_n = 1.0f / (float)P.total;
    // The round-2 MFMA kernel (DAAM_NO_PIPE_FINALIZE=1) walks a host-built chunk table of at most kFinMaxChunks chunks x 2 key
    // lanes x 64 keys, so a larger class goes out as several launches over key sub-ranges (kFinMfmaKeysPerLaunch each, every one
    // with its own chunk table) -- the pipelined kernel, the LDS kernel and the other classes take any key count.
    constexpr int kFinMfmaKeysPerLaunch = kFinMaxChunks * 128;
    std::vector<FinLaunch> up_parts;
    if (P.mfma_up && !P.pipe_up) {
        FinLaunch U = fin_class_launch(c, P, 1, T.dev, out);
        U.inv_n = inv_n;
        U.mfma_ops = c->d_up32_ops;
        for (int begin = 0; begin < P.n[1]; begin += kFinMfmaKeysPerLaunch) {
            FinLaunch part = U;
            part.keys = U.keys + begin;
            part.n_keys = std::min(kFinMfmaKeysPerLaunch, P.n[1] - begin);
            part.n_chunks = std::min(fin_chunks(1, part.n_keys, rows), kFinMaxChunks);
            finalize_chunk_ranges(part.n_keys, part.n_chunks, &part);
            up_parts.push_back(part);
        }
    }
    // SDXL-1024 in fp16: the same-size and the x2 class side by side in ONE launch
    const bool paired = up_parts.size() == 1 && P.have[0] && !c->no_paired_finalize;
    if (paired) P.have[0] = false;
    const std::string dt = dtype_name(dtype);
    return fin_launch_classes(c, P, dtype, s, "finalize", "", [&](int cls, hipStream_t ks, int* grid, int* lds, std::string* name) -> hipError_t {
        if (cls == 1 && P.pipe_up) {
            FinPipeLaunch PL = fin_pipe_launch(c, P, dtype, T.dev, out);
            PL.inv_n = inv_n;
            *name = fin_name("finalize_up32_pipe_kernel", dt + (P.fold_same ? " + same-size keys" : ""));
            return launch_finalize_up32_pipe(PL, nullptr, 1, dtype, ks, grid);
        }
        FinLaunch L = fin_class_launch(c, P, cls, T.dev, out);
        L.inv_n = inv_n;
        if (cls == 1 && paired) {
            *name = fin_name("finalize_up32_same_kernel", "f16");
            FinLaunch same = fin_class_launch(c, P, 0, T.dev, out);
            same.inv_n = inv_n;
            return launch_finalize_up32_same(up_parts[0], same, ks, grid);
        }
        if (cls == 1 && P.mfma_up) {
            *name = fin_name("finalize_up32_mfma_kernel", "f16");
            hipError_t e = hipSuccess;
            for (size_t part = 0; part < up_parts.size() && e == hipSuccess; ++part) {
                int g = 0;
                e = launch_finalize_up32_mfma(up_parts[part], ks, &g);
                *grid += g;
            }
            return e;
        }
        return fin_launch_class(cls, L, nullptr, 1, dtype, ks, grid, lds, name);
    });
}

// N global heat maps, one launch per class on the *_grouped_kernel forms, over the planes of `layers[0, n_layers)` (plane dtype
// `dtype`): key i of that table belongs to group key_group[i].  The per-group part of a launch (key range, rows, 1/N, output
// base, pointer-table offsets) travels in the kernel arguments and blockIdx.z selects it.  Arguments validated by the caller.
// per_group_fallback: the round-2 MFMA x2 kernel (DAAM_NO_PIPE_FINALIZE) may serve the call as one daam_finalize per group (only
// over the context's own sums); otherwise such keys take the grouped LDS kernel.  prefix: what the caller launched ahead of
// this inside the profiled span it opened (none: the span starts here).
int fin_grouped(DaamCtx* c, Layer* layers, int n_layers, int dtype, const int32_t* key_group, int total_keys, int n_groups,
                const int32_t* n_rows, const int* rows, float* out, size_t group_stride, hipStream_t s, bool per_group_fallback,
                const std::string& prefix)
{
    int rc = fin_zero_owed(layers, (size_t)n_layers, s);
    if (rc) return rc;
    if (c->rect()) return fin_rect(c, layers, n_layers, dtype, nullptr, key_group, n_groups, rows, out, group_stride, s);
    FinPlan P;
    if ((rc = fin_plan(c, layers, n_layers, dtype, nullptr, key_group, n_groups, rows, P))) return rc;
    if (P.mfma_up && !P.pipe_up && per_group_fallback) {
        std::vector<uint8_t> mask(total_keys);
        for (int g = 0; g < n_groups; ++g) {
            for (int i = 0; i < total_keys; ++i) mask[i] = key_group[i] == g;
            if ((rc = daam_finalize(c, mask.data(), n_rows[g], out + (size_t)g * group_stride, s))) return rc;
        }
        return 0;
    }
    if (c->profile && prefix.empty()) (void)hipEventRecord(c->prof_event(1, 0), s);
    FinTables T(c, s);
    if ((rc = T.put(P.tab, T.hit(P.tab), nullptr, 0))) return rc;
    // the output is accumulated with atomics: rows [0, rows[g]) of every group are cleared first
    hipError_t ze = launch_zero_groups(out, group_stride, c->out_side * c->out_side, rows, n_groups, s);
    if (ze != hipSuccess) return fail((int)ze, "output zeroing: %s", hipGetErrorString(ze));
    auto groups_of = [&](int cls, FinGroup* G) {
        for (int g = 0; g < n_groups; ++g) {
            FinGroup& q = G[g];
            q.key_begin = P.begin[cls][g];
            q.n_keys = P.count[cls][g];
            q.rows = rows[g];
            q.inv_n = 1.0f / (float)P.n_of[g];
            q.out_off = (int64_t)((size_t)g * group_stride);
            q.ptr_off = (int32_t)(g * P.ptr_per_group);
            q.same_off = (int32_t)(g * P.same_per_group);
        }
    };
    const std::string dt = dtype_name(dtype);
    return fin_launch_classes(c, P, dtype, s, "grouped finalize", prefix, [&](int cls, hipStream_t ks, int* grid, int* lds, std::string* name) -> hipError_t {
        if (cls == 1 && P.pipe_up) {
            FinPipeGroupLaunch PG;
            memset(&PG, 0, sizeof PG);
            PG.L = fin_pipe_launch(c, P, dtype, T.dev, out);
            groups_of(1, PG.g);
            *name = fin_name("finalize_up32_pipe_grouped_kernel", dt + (P.fold_same ? " + same-size keys" : ""));
            return launch_finalize_up32_pipe(PG.L, &PG, n_groups, dtype, ks, grid);
        }
        FinGroupLaunch G;
        memset(&G, 0, sizeof G);
        G.L = fin_class_launch(c, P, cls, T.dev, out);
        groups_of(cls, G.g);
        return fin_launch_class(cls, G.L, &G, n_groups, dtype, ks, grid, lds, name);
    });
}

// The argument checks daam_finalize_groups and daam_finalize_bins share (the NULL checks aside).  bin_begin / bin_end: the
// window range of every group (NULL: none given); group_set: see daam_finalize_bins (NULL: the keys of group g carry g).
// Fills rows[g] and the key count of the context.
int fin_check_groups(DaamCtx* c, const int32_t* key_group, int n_groups, const int32_t* group_set, const int32_t* bin_begin,
                     const int32_t* bin_end, const int32_t* n_rows, size_t group_stride, int* rows, int* total_keys)
{
    if (n_groups < 1 || n_groups > kFinMaxGroups) return fail(DAAM_E_INVALID, "n_groups %d not in 1..%d", n_groups, kFinMaxGroups);
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "finalize with deferred taps pending: flush first");
    const int nb = std::max(1, c->n_bins);
    int n_sets = group_set ? 0 : n_groups;
    for (int g = 0; g < n_groups; ++g) {
        if (bin_begin && (bin_begin[g] < 0 || bin_end[g] > nb || bin_begin[g] >= bin_end[g]))
            return fail(DAAM_E_INVALID, "group %d: window range [%d, %d) not a non-empty part of [0, %d)", g, bin_begin[g], bin_end[g], nb);
        if (group_set) {
            if (group_set[g] < 0) return fail(DAAM_E_INVALID, "group_set[%d] = %d < 0", g, group_set[g]);
            n_sets = std::max(n_sets, group_set[g] + 1);
        }
    }
    daam_key_offset(c, 0, nullptr, total_keys);
    for (int g = 0; g < n_groups; ++g) rows[g] = fin_rows(c, n_rows[g]);
    const size_t plane = (size_t)c->out_h * c->out_w;
    for (int g = 0; g + 1 < n_groups; ++g)
        if (group_stride < (size_t)rows[g] * plane)
            return fail(DAAM_E_INVALID, "group_stride %zu < %d rows of %zu floats: groups would overlap", group_stride, rows[g], plane);
    std::vector<int> per_set(n_sets, 0);
    for (int i = 0; i < *total_keys; ++i) {
        const int k = key_group[i];
        // (with group_set: keys of a set no group takes are simply not selected)
        if (k < -1 || (!group_set && k >= n_sets)) return fail(DAAM_E_INVALID, "key_group[%d] = %d not in -1..%d", i, k, n_sets - 1);
        if (k >= 0 && k < n_sets) ++per_set[k];
    }
    for (int g = 0; g < n_groups; ++g)
        if (!per_set[group_set ? group_set[g] : g]) return fail(DAAM_E_NOMAPS, "no heat maps selected for group %d", g);
    return 0;
}

}  // namespace

extern "C" {

int daam_finalize_prepare(DaamCtx* c, const uint8_t* key_mask, int n_rows, float* out, void* stream)
{
    if (!c || !out) return fail(DAAM_E_INVALID, "NULL argument");
    if (c->n_bins > 1) return fail(DAAM_E_UNSUPPORTED, "daam_finalize_prepare: not on a time-binned context (daam_finalize_bins)");
    if (c->rect()) return fail(DAAM_E_UNSUPPORTED, "daam_finalize_prepare: not on a context with an output or a layer of unequal sides");
    DeviceGuard on_device(c);
    hipStream_t s = (hipStream_t)stream;
    const int rows = fin_rows(c, n_rows);
    c->prep_out = c->fold_out = nullptr;
    c->prep_rows = rows;
    if (c->no_fin_cache || !fin_out_zeroable(c, out, rows)) return 0;  // daam_finalize does everything itself
    FinPlan P;
    if (fin_plan(c, c->layers.data(), c->max_layers, c->acc_dtype, key_mask, nullptr, 1, &rows, P)) return 0;   // nothing selected / unsupported: daam_finalize reports it
    const size_t out_bytes = sizeof(float) * rows * (size_t)c->out_side * c->out_side;
    FinTables T(c, s);
    const bool hit = T.hit(P.tab);
    if (!hit && !T.cacheable(P.tab)) return 0;
    if (hit && !c->pending.empty()) {                            // the table-upload kernel of the coming tap launch clears `out`
        c->fold_out = out;
        c->fold_bytes = out_bytes;
        c->fold_stream = s;
        return 0;
    }
    int rc = T.put(P.tab, hit, out, out_bytes);                  // (first call of a geometry / selection: tables + zeroing now)
    if (rc) return rc;
    c->prep_out = out;
    c->prep_stream = s;
    return 0;
}

int daam_finalize(DaamCtx* c, const uint8_t* key_mask, int n_rows, float* out, void* stream)
{
    if (!c || !out) return fail(DAAM_E_INVALID, "NULL argument");
    if (!c->pending.empty()) return fail(DAAM_E_STATE, "finalize with deferred taps pending: flush first");
    if (c->n_bins > 1) {                                       // a binned context: the whole generation = windows [0, n_bins)
        int total = 0;
        daam_key_offset(c, 0, nullptr, &total);
        std::vector<int32_t> kg(total > 0 ? total : 1, -1);
        for (int i = 0; i < total; ++i) kg[i] = (!key_mask || key_mask[i]) ? 0 : -1;
        const int32_t b0 = 0, b1 = c->n_bins, r = n_rows;
        return daam_finalize_bins(c, kg.data(), 1, nullptr, &b0, &b1, &r, out, 0, stream);
    }
    DeviceGuard on_device(c);
    return fin_single(c, key_mask, nullptr, n_rows, out, (hipStream_t)stream);
}

int daam_finalize_groups(DaamCtx* c, const int32_t* key_group, int n_groups, const int32_t* n_rows, float* out,
                         size_t group_stride, void* stream)
{
    if (!c || !out || !key_group || !n_rows) return fail(DAAM_E_INVALID, "NULL argument");
    int rows[kFinMaxGroups], total_keys = 0;
    int rc = fin_check_groups(c, key_group, n_groups, nullptr, nullptr, nullptr, n_rows, group_stride, rows, &total_keys);
    if (rc) return rc;
    if (c->n_bins > 1) {                                       // a binned context: every group over the whole generation
        std::vector<int32_t> b0(n_groups, 0), b1(n_groups, c->n_bins);
        return daam_finalize_bins(c, key_group, n_groups, nullptr, b0.data(), b1.data(), n_rows, out, group_stride, stream);
    }
    DeviceGuard on_device(c);
    hipStream_t s = (hipStream_t)stream;
    if (n_groups == 1) return fin_single(c, nullptr, key_group, n_rows[0], out, s);
    c->prep_out = c->fold_out = nullptr;
    return fin_grouped(c, c->layers.data(), c->max_layers, c->acc_dtype, key_group, total_keys, n_groups, n_rows, rows, out, group_stride,
                       s, true, "");
}

// daam_finalize_bins: daam_finalize_groups with a window range per group.  Groups that each take ONE window (and no two of them
// the same key of the same window) run the grouped class kernels straight on the windows' planes: the key space of the call is
// the window slots' (window-major), and the per-group key table points at window bin_begin[g].  Otherwise one launch of
// finalize_bin_sum_kernel adds every selected key's windows [bin_begin[g], bin_end[g]) into f32 scratch planes (rows
// [0, n_rows[g]) only) and the grouped class kernels run on those, dispatched on THEIR dtype (f32).
int daam_finalize_bins(DaamCtx* c, const int32_t* key_group, int n_groups, const int32_t* group_set, const int32_t* bin_begin,
                       const int32_t* bin_end, const int32_t* n_rows, float* out, size_t group_stride, void* stream)
{
    if (!c || !out || !key_group || !bin_begin || !bin_end || !n_rows) return fail(DAAM_E_INVALID, "NULL argument");
    int rows[kFinMaxGroups], total_keys = 0;
    int rc = fin_check_groups(c, key_group, n_groups, group_set, bin_begin, bin_end, n_rows, group_stride, rows, &total_keys);
    if (rc) return rc;
    const int nb = std::max(1, c->n_bins);
    auto set_of = [&](int g) { return group_set ? group_set[g] : g; };
    bool direct = true;
    for (int g = 0; g < n_groups && direct; ++g) {
        direct = bin_end[g] - bin_begin[g] == 1;
        for (int h = 0; h < g && direct; ++h) direct = !(bin_begin[h] == bin_begin[g] && set_of(h) == set_of(g));
    }
    if (direct && nb == 1 && !group_set) return daam_finalize_groups(c, key_group, n_groups, n_rows, out, group_stride, stream);
    if (c->rect() && (nb > 1 || !direct))
        return fail(DAAM_E_UNSUPPORTED, "daam_finalize_bins: no window ranges on a context with an output or a layer of unequal sides");
    DeviceGuard on_device(c);
    hipStream_t s = (hipStream_t)stream;
    c->prep_out = c->fold_out = nullptr;
    if (direct) {
        // key (window b, key i) of the slots' key space = b * total_keys + i
        const size_t ext = (size_t)nb * total_keys;
        std::vector<int32_t> kg(ext > 0 ? ext : 1, -1);
        for (int g = 0; g < n_groups; ++g)
            for (int i = 0; i < total_keys; ++i)
                if (key_group[i] == set_of(g)) kg[(size_t)bin_begin[g] * total_keys + i] = g;
        return fin_grouped(c, c->layers.data(), nb * c->max_layers, c->acc_dtype, kg.data(), (int)ext, n_groups, n_rows, rows, out,
                           group_stride, s, false, "");
    }
    // ---- window-range reduction: one task per (group, selected key)
    std::vector<std::pair<int, int>> key_at;                  // key i -> (layer, head)
    for (int l = 0; l < c->max_layers; ++l)
        if (c->layers[l].configured)
            for (int h = 0; h < c->layers[l].heads; ++h) key_at.push_back({l, h});
    const size_t elem = acc_elem(c->acc_dtype);
    const int per_tile = bin_sum_elems_per_tile(c->acc_dtype);
    std::vector<BinSumTask> tasks;
    std::vector<Layer> vl;                                     // the scratch planes as one-head layers
    std::vector<int32_t> vg;
    size_t scratch = 0;
    int tiles = 0;
    for (int g = 0; g < n_groups; ++g)
        for (int i = 0; i < total_keys; ++i) {
            if (key_group[i] != set_of(g)) continue;
            const Layer& l = c->layers[(size_t)bin_begin[g] * c->max_layers + key_at[i].first];
            BinSumTask t;
            memset(&t, 0, sizeof t);
            t.src = static_cast<const char*>(l.acc) + (size_t)key_at[i].second * c->tokens * l.hw * elem;
            t.dst = reinterpret_cast<float*>(scratch);             // offset for now
            t.win_stride = (int64_t)(l.bytes / elem);
            t.n_elem = (int64_t)rows[g] * l.hw;
            t.n_win = bin_end[g] - bin_begin[g];
            t.tile_begin = tiles;
            t.vec = ((reinterpret_cast<uintptr_t>(t.src) | l.bytes) & 15) == 0;
            tiles += (int)((t.n_elem + per_tile - 1) / per_tile);
            tasks.push_back(t);
            Layer v;
            v.configured = true;
            v.heads = 1;
            v.side = l.side;
            v.hw = l.hw;
            v.factor = l.factor;
            v.tab = l.tab;
            v.bytes = (size_t)t.n_elem * sizeof(float);
            vl.push_back(v);
            vg.push_back(g);
            scratch += (v.bytes + 255) & ~size_t(255);
        }
    if (scratch > c->bin_scratch_bytes) {
        if (c->bin_scratch) {
            HIP_TRY(hipDeviceSynchronize());                   // earlier finalize calls may still read the old scratch
            HIP_TRY(hipFree(c->bin_scratch));
            c->bin_scratch = nullptr;
            c->bin_scratch_bytes = 0;
        }
        HIP_TRY(hipMalloc(&c->bin_scratch, scratch));
        c->bin_scratch_bytes = scratch;
    }
    for (size_t j = 0; j < tasks.size(); ++j) {
        tasks[j].dst = reinterpret_cast<float*>(static_cast<char*>(c->bin_scratch) + reinterpret_cast<size_t>(tasks[j].dst));
        tasks[j].vec = tasks[j].vec && (reinterpret_cast<uintptr_t>(tasks[j].dst) & 15) == 0;
        vl[j].acc = tasks[j].dst;
    }
    // the windows' sums must hold what they should: a zeroing still owed since daam_reset comes first
    for (int g = 0; g < n_groups; ++g)
        for (int b = bin_begin[g]; b < bin_end[g]; ++b)
            for (int l = 0; l < c->max_layers; ++l) {
                int zrc = ensure_zeroed(c->layers[(size_t)b * c->max_layers + l], s);
                if (zrc) return zrc;
            }
    const size_t tab_bytes = tasks.size() * sizeof(BinSumTask);
    if (tab_bytes > Ring::kBytes) return fail(DAAM_E_UNSUPPORTED, "%zu window-range tasks in one call", tasks.size());
    if (c->profile) (void)hipEventRecord(c->prof_event(1, 0), s);   // timed: the reduction and the class kernels
    {
        FinTables T(c, s);                                     // the task table: a ring region until the reduction has run
        if ((rc = T.upload(tasks.data(), tab_bytes, nullptr, nullptr, 0))) return rc;
        BinSumLaunch BL;
        BL.tasks = reinterpret_cast<const BinSumTask*>(T.dev);
        BL.n_tasks = (int32_t)tasks.size();
        BL.n_tiles = tiles;
        hipError_t e = launch_finalize_bin_sum(BL, c->acc_dtype, s);
        if (e != hipSuccess) return fail((int)e, "window-range reduction: %s", hipGetErrorString(e));
    }
    return fin_grouped(c, vl.data(), (int)vl.size(), DAAM_F32, vg.data(), (int)vg.size(), n_groups, n_rows, rows, out, group_stride, s,
                       false, std::string("finalize_bin_sum_kernel<") + dtype_name(c->acc_dtype) + ">");
}

}  // extern "C"
