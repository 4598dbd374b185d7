// Body of tap_d64_kernel (daam_tap_d64.hip), included once per step protocol: the includer is a __global__ function template with
// IN, ACC_T, FAST_EXP, FULL64, WAVES and the kernel argument `const TapLaunch L` in scope, and a compile-time bool COUNTED.
    static_assert(!COUNTED || FULL64, "counted waits: the DMA path only");
    constexpr int NT = 64 * WAVES;                            // threads per workgroup
    constexpr int TILE = 32 * WAVES;                          // pixels per workgroup (the host sizes tiles_per_head with it)
    static_assert(WAVES == 4 || (WAVES == 8 && FULL64), "eight waves: head_dim-64 launches (the DMA path) only");
    constexpr int KCH = (kTok * 8 + 255) / 256;               // 16-B K pieces per thread per step (3)
    constexpr int VEC = AccVec<ACC_T>::kPerVec;
    constexpr int PPR = TILE / VEC;
    constexpr size_t kPtrOff = tap_d64_lds_bytes<ACC_T, WAVES>() - (size_t)kMaxStepsPerLaunch * 2 * sizeof(void*);

    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* kbuf = smem;                               // [2][kTapKBuf], then the four waves' Q tiles
    ACC_T* stage = reinterpret_cast<ACC_T*>(smem);            // [kTok][TILE], aliases both
    const void** sptr = reinterpret_cast<const void**>(smem + kPtrOff);

    const int wg = mfma_logical_block(L.total_wgs, L.wgs_per_xcd);
    if (wg < 0) return;
    tap_mark_started(L);
    TapLayer lay;
    const bool table = L.layers != nullptr;
    if (table) {
        const DAAM_GLOBAL TapLayer* gl = as_global<TapLayer>(L.layers);
        load_layer(gl + mfma_find_layer(gl, L.n_layers, wg), &lay);
    } else {
        lay = L.one;
    }
    const int tid = threadIdx.x;
    tap_step_ptrs_to_lds<NT>(L, lay, table, sptr, tid);
    const int n_steps = lay.n_steps;
    const TapTile tile = tap_tile_decode<TILE>(lay, wg);
    const int kh = tile.kh, p0 = tile.p0;
    const int64_t k_off = tile.k_off, q_off = tile.q_off;

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the DMA block choice must not become exec masks
    const int j = lane & 15, h = lane >> 4;

    // ---- running sums -> registers (through the staging tile, 16-byte row pieces) --------------
    // (text in every kernel that has it: as functions shared through daam_tap_tile64.h it changed each of d64, pair, chunk, wide and mfma)
    typename Pair<ACC_T>::T run0[kSlots16 / 2], run1[kSlots16 / 2];   // slot pairs (2i, 2i+1)
    ACC_T* acc = reinterpret_cast<ACC_T*>(lay.acc) + (size_t)kh * kTok * lay.hw;
    if (!lay.fresh) {
        for (int piece = tid; piece < kTok * PPR; piece += NT) {
            const int row = piece / PPR, col = (piece - row * PPR) * VEC;
            if (p0 + col < lay.hw)
                *reinterpret_cast<float4v*>(stage + row * TILE + col) =
                    *as_global<float4v>(acc + (size_t)row * lay.hw + p0 + col);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSlots16; ++i) {
            const int t = slot16_token(i, h);
            if (t < kTok) {
                run0[i >> 1][i & 1] = from_acc<ACC_T>(stage[t * TILE + wave * 32 + j]);
                run1[i >> 1][i & 1] = from_acc<ACC_T>(stage[t * TILE + wave * 32 + 16 + j]);
            } else {
                run0[i >> 1][i & 1] = 0;
                run1[i >> 1][i & 1] = 0;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kSlots16; ++i) { run0[i >> 1][i & 1] = 0; run1[i >> 1][i & 1] = 0; }
    }
    __syncthreads();                                          // staging reads done; sptr visible
    // head_dim < 64 (multiple of 8; SD-v1.5's 40): the contraction runs over 64 with zeros beyond head_dim --
    // K chunks past it are never written (the buffers are zeroed once), Q chunks past it are fetched from a valid
    // address and cleared before they are written to LDS.
    const int d = lay.head_dim;
    const bool partial = !FULL64 && d < 64;                   // wave-uniform
    if (partial) {
        for (int i = tid; i < 2 * kTapKBuf / 16; i += NT)
            *reinterpret_cast<float4v*>(kbuf + i * 16) = float4v{0, 0, 0, 0};
        __syncthreads();                                      // the first K tile lands on top of the zeros
    } else {
        tap64_zero_pad_rows<NT>(kbuf, tid);
    }

    // per-thread K piece coordinates: piece c = tid + 256 j2 -> row t = c / 8 = (tid >> 3) + 32 j2, chunk c % 8.  The swizzle
    // key ((t >> 1) & 7) and the validity of the chunk do not depend on j2, so ONE LDS offset (+ 4096 j2) and ONE global
    // offset (+ 32 rows for piece 1, folded into the scalar base; piece 2 has its own, because the threads whose row would
    // be 77..95 re-read their piece 0 instead) serve the three pieces.
    static_assert(KCH == 3, "three K pieces per thread");
    const int k_t = tid >> 3, k_ch = tid & 7;
    const bool k_in_row = k_ch * 8 < d;                       // chunk inside the head's d elements
    const bool k_row2 = k_t + 64 < kTok;                      // piece 2 exists
    const unsigned k_src0 = (unsigned)((k_t * (int)lay.k_st + (k_in_row ? k_ch * 8 : 0)) * 2);
    const int k_dst0 = k_t * kTapRow + swz_chunk(k_t, k_ch);
    const unsigned k_step = (unsigned)__builtin_amdgcn_readfirstlane(32 * (int)lay.k_st * 2);   // bytes per 32 K rows
    const unsigned k_src2 = k_row2 ? k_src0 + 2 * k_step : k_src0;
    // Q pieces of this lane: piece p = lane + 64 i (i = 0..3) of the wave's 32 pixel rows -> row = p >> 3 = (lane >> 3) + 8 i,
    // chunk = lane & 7.  Addresses = wave-uniform base (the step's tensor pointer, made an SGPR pair by readfirstlane; + 8 i
    // pixel rows for piece i) + ONE 32-bit per-lane byte offset that never changes.  tap_d64_supported() keeps every
    // offset below 2^31.
    const int q_row = lane >> 3, q_chunk = lane & 7;
    const bool q_valid = q_chunk * 8 < d;
    const unsigned q_co = q_valid ? q_chunk * 16 : 0;
    const int q_px = p0 + wave * 32 + q_row;
    const unsigned q_b0 = (unsigned)((q_off + (int64_t)min(q_px, lay.hw - 1) * lay.q_sp) * 2) + q_co;
    // piece i sits 8 i pixel rows further: a wave-uniform byte step added to the scalar base.  hw is a multiple of 8
    // (tap_d64_supported), so a piece is inside the layer for all of its lanes or for none; a piece outside re-reads piece 0's
    // rows (or, when the whole wave is outside, the layer's last row: q_b0 is clamped) and its results are never stored.
    const int q_rows_in = __builtin_amdgcn_readfirstlane(lay.hw - (p0 + wave * 32));
    const unsigned q_step8 = (unsigned)__builtin_amdgcn_readfirstlane(8 * (int)lay.q_sp * 2);   // bytes per 8 pixel rows
    unsigned q_s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q_s[i] = 8 * i < q_rows_in ? (unsigned)i * q_step8 : 0u;
    // LDS write position of piece i: row (q_row + 8 i), swizzle key ((lane >> 4) + 4 i) & 7 = (lane >> 4) ^ 4 (i & 1)
    unsigned char* qtile = kbuf + kTapQOff + wave * kTapQTile;
    const int q_wr = q_row * kTapRow + ((q_chunk ^ (lane >> 4)) << 4);
    // operand reads: row l&15 of a 16-row tile, chunk 4 ks + (l >> 4); the same offset serves K (A) and Q (B)
    const int f_rd = j * kTapRow + swz_chunk(j, h);            // k-step 1: ^ 64 (not a function of its own: that folds the swizzle differently)
    const unsigned k_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(k_off * 2));

    float4v kreg[KCH];
    auto issue_k = [&](int s) {
        const __amdgpu_buffer_rsrc_t kt = tap_tensor_rsrc(sptr[2 * s + 1]);
        kreg[0] = __builtin_bit_cast(float4v, __builtin_amdgcn_raw_buffer_load_b128(kt, k_src0, k_base, 0));
        kreg[1] = __builtin_bit_cast(float4v, __builtin_amdgcn_raw_buffer_load_b128(kt, k_src0, k_base + k_step, 0));
        kreg[2] = __builtin_bit_cast(float4v, __builtin_amdgcn_raw_buffer_load_b128(kt, k_src2, k_base, 0));
    };
    auto commit_k = [&](int buf) {
        unsigned char* kb = kbuf + buf * kTapKBuf + k_dst0;
        if (k_in_row) {
            *reinterpret_cast<float4v*>(kb) = kreg[0];
            *reinterpret_cast<float4v*>(kb + 32 * kTapRow) = kreg[1];
            if (k_row2) *reinterpret_cast<float4v*>(kb + 64 * kTapRow) = kreg[2];
        }
    };
    float4v qreg[4];
    auto issue_q = [&](int s) {
        const __amdgpu_buffer_rsrc_t qt = tap_tensor_rsrc(sptr[2 * s]);
#pragma unroll
        for (int i = 0; i < 4; ++i) qreg[i] = __builtin_bit_cast(float4v, __builtin_amdgcn_raw_buffer_load_b128(qt, q_b0, q_s[i], 0));
    };
    auto commit_q = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4v v = (partial && !q_valid) ? float4v{0, 0, 0, 0} : qreg[i];
            *reinterpret_cast<float4v*>(qtile + i * 8 * kTapRow + (q_wr ^ (64 * (i & 1)))) = v;
        }
    };

    // LDS-DMA form (FULL64 launches only).  K: 1 KiB block blk = WAVES j2 + wave (10 blocks: rows 8 blk .. 8 blk + 7; rows 77..79 re-read
    // row 76: finite, their logits are masked); lane -> row 8 blk + (lane >> 3), LDS chunk slot lane & 7 = source chunk
    // (lane & 7) ^ ((row >> 1) & 7).  Q: block i = rows 8 i .. 8 i + 7 of the wave's 32, same rule.
    unsigned kd_src[3];
#pragma unroll
    for (int j2 = 0; j2 < 3; ++j2) {
        const int blk = WAVES * j2 + wave;
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
    // (text, as in walk: through tap64_dma_k every head_dim-64 instance is scheduled differently; pair calls it)
    auto dma_k = [&](int s, int buf) {
        const __amdgpu_buffer_rsrc_t kt = tap_tensor_rsrc(sptr[2 * s + 1]);
#pragma unroll
        for (int j2 = 0; j2 < 3; ++j2) {
            const int blk = WAVES * j2 + wave;                // wave-uniform
            // COUNTED: a block that every wave / no wave has is decided here, so that one scalar branch per step remains
            const bool every = COUNTED && WAVES * j2 + WAVES - 1 < 10, none = COUNTED && WAVES * j2 >= 10;   // constants once unrolled
            if (every || (!none && blk < 10))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(kt, (lds_ptr_t)(kbuf + buf * kTapKBuf + blk * 1024), 16, kd_src[j2], k_base, 0, 0);
        }
    };
    auto dma_q = [&](int s) { tap64_dma_q(sptr[2 * s], qtile, qd_src, q_s); };
    const floatx4 cmask = premask_tile4(h);
    // one denoising step: logits of step s from the K and Q tiles in LDS, then the fetches of the next step (head_dim 64: by DMA
    // into the other K buffer / this wave's own Q tile, whose reads are behind it; head_dim < 64: step s + 1 from the staging
    // registers into LDS and the request for step s + 2), softmax + accumulate of the two pixel groups
    // COUNTED: K DMAs per wave and step = blocks WAVES j2 + wave < 10: the first 10 % WAVES waves have one more than the others
    constexpr int NK_LO = 10 / WAVES;
    const bool k_hi = wave < 10 % WAVES;                      // wave-uniform (scalar branch around an immediate wait count)
    auto step = [&](int s) {
        if constexpr (!COUNTED) __syncthreads();
        const unsigned char* kb = kbuf + (s & 1) * kTapKBuf;
        [[maybe_unused]] const int s_fetch = min(s + 1, n_steps - 1);   // branch-free: the last step re-fetches itself
        // the K buffer of step s + 1 was last read in step s - 1 and every wave is past this step's barrier: its DMAs go out first
        if constexpr (FULL64) dma_k(s_fetch, (s + 1) & 1);
        if constexpr (COUNTED) {
            // this wave's Q(s): at most the K DMAs just issued stay outstanding
            if (k_hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NK_LO + 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NK_LO) : "memory");
        }
        const half8 q00 = *reinterpret_cast<const half8*>(qtile + f_rd), q01 = *reinterpret_cast<const half8*>(qtile + (f_rd ^ 64));
        const half8 q10 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + f_rd);
        const half8 q11 = *reinterpret_cast<const half8*>(qtile + 16 * kTapRow + (f_rd ^ 64));
        if constexpr (FULL64) {
            // this wave's Q tile is free once its four operand reads have returned: the next step's rows are requested BEFORE the MFMAs
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            dma_q(s_fetch);
        }
        floatx4 c0[5], c1[5];
        tap64_mfma_chain<IN>(kb, f_rd, q00, q01, q10, q11, cmask, c0, c1);
        if constexpr (!FULL64) {
            // head_dim < 64 (register-staged): the pieces of step s + 1 were requested a whole step ago -- into LDS now (K buffer
            // (s + 1) & 1 was last read in step s - 1, which every wave left before this step's barrier; the Q tile is this wave's
            // own and its operand reads are behind it), then the request for step s + 2 goes out: a fetch has a whole step to
            // land instead of one softmax (SD-v1.5's 64 x 64 layers: 330 -> 285 us per 50-step launch)
            commit_k((s + 1) & 1);
            commit_q();
            issue_k(min(s + 2, n_steps - 1));                 // branch-free: the last steps re-fetch the last one
            issue_q(min(s + 2, n_steps - 1));
        }
        tap_softmax_accumulate<IN, ACC_T, FAST_EXP>(c0, lay, h, run0);
        tap_softmax_accumulate<IN, ACC_T, FAST_EXP>(c1, lay, h, run1);
        if constexpr (COUNTED) {
            // invariants (i) and (ii): this wave's K(s + 1) pieces have landed (only the four Q(s + 1) DMAs may be outstanding), its K(s)
            // reads are done; Q(s + 1) stays in flight across the barrier
            asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else if constexpr (FULL64) {
            // this wave's DMAs have landed; the next step's barrier publishes K
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    };
    if constexpr (COUNTED) {
        dma_k(0, 0);
        dma_q(0);
        asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // K(0) is in LDS; Q(0) is waited for in step 0
    } else if constexpr (FULL64) {
        dma_k(0, 0);
        dma_q(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        issue_k(0);
        issue_q(0);
        commit_k(0);
        commit_q();
        issue_k(min(1, n_steps - 1));
        issue_q(min(1, n_steps - 1));
    }
    for (int s = 0; s < n_steps; ++s) step(s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // nothing of the last (redundant) fetches is in flight any more
    __syncthreads();                                          // all K reads done before the staging tile reuses the space

    // ---- write back: registers -> LDS [token][pixel] -> 16-byte row pieces -------------------
#pragma unroll
    for (int i = 0; i < kSlots16; ++i) {
        const int t = slot16_token(i, h);
        if (t < kTok) {
            stage[t * TILE + wave * 32 + j] = to_acc<ACC_T>(run0[i >> 1][i & 1]);
            stage[t * TILE + wave * 32 + 16 + j] = to_acc<ACC_T>(run1[i >> 1][i & 1]);
        }
    }
    __syncthreads();
    for (int piece = tid; piece < kTok * PPR; piece += NT) {
        const int row = piece / PPR, col = (piece - row * PPR) * VEC;
        if (p0 + col < lay.hw)
            *as_global_rw<float4v>(acc + (size_t)row * lay.hw + p0 + col) =
                *reinterpret_cast<const float4v*>(stage + row * TILE + col);
    }
