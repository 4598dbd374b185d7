// body of finalize_up_kernel and of its grouped form (daam_finalize_groups); included inside the kernel, where `L` is the launch
    constexpr int O = 64;
    constexpr int R = O / S;                                  // 2 or 4: weights repeat with period R
    using P = Plane<ACC_T>;
    constexpr int NP = S * S / P::kPerPiece;                  // 16-byte pieces per plane
    constexpr int PL = (NP + 63) / 64;                        // pieces per lane

    __shared__ __align__(16) float planes[4][S * S];
    __shared__ __align__(16) float red[2 * O * O];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tok = blockIdx.x;

    const int tab = L.keys[0].tab;                            // one map size per launch
    const int16_t* tix = L.tab_idx + (size_t)tab * O * 4;
    const float* tw = L.tab_w + (size_t)tab * O * 4;
    const float* my = planes[wave];
    const float* x0 = my + tix[lane * 4 + 0];
    const float* x1 = my + tix[lane * 4 + 1];
    const float* x2 = my + tix[lane * 4 + 2];
    const float* x3 = my + tix[lane * 4 + 3];
    const float wx0 = tw[lane * 4 + 0], wx1 = tw[lane * 4 + 1], wx2 = tw[lane * 4 + 2], wx3 = tw[lane * 4 + 3];

    // this lane's output column: acc2[i] = rows (P0 + 2i, P0 + 2i + 1); with P0 = 1 rows 0 and 63 in edge[]
    constexpr int P0 = (R == 2) ? 1 : 0;
    static_assert(src_floor<S, O>(P0) == src_floor<S, O>(P0 + 1), "paired output rows must share their taps");
    float2v acc2[O / 2];
    float edge[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < O / 2; ++i) acc2[i] = float2v{0.f, 0.f};

    // this wave's keys: first, first + stride, ...   Their plane base pointers go to LDS once
    // (no dependent table fetch per key), and the planes are fetched kDepth keys ahead: a wave's
    // critical path is then one HBM latency per kDepth planes instead of two per plane.
    constexpr int kDepth = 4;
    constexpr int kMaxKeysPerWave = 64;
    __shared__ const void* kbase[4][kMaxKeysPerWave];
    const int stride = gridDim.y * 4;
    const int first = blockIdx.y * 4 + wave;
    const int nk = first < L.n_keys ? min((L.n_keys - first + stride - 1) / stride, kMaxKeysPerWave) : 0;
    if (lane < nk) kbase[wave][lane] = as_global<FinKey>(L.keys)[first + lane * stride].base;
    __builtin_amdgcn_wave_barrier();
    typename P::Piece pre[kDepth][PL];
    auto fetch = [&](int i, typename P::Piece (&dst)[PL]) {
        const ACC_T* src = reinterpret_cast<const ACC_T*>(kbase[wave][i]) + (size_t)tok * S * S;
#pragma unroll
        for (int j = 0; j < PL; ++j) {
            const int piece = lane + 64 * j;
            if (piece < NP) dst[j] = *as_global<typename P::Piece>(src + piece * P::kPerPiece);
        }
    };
#pragma unroll
    for (int d = 0; d < kDepth; ++d)
        if (d < nk) fetch(d, pre[d]);
    for (int i0 = 0; i0 < nk; i0 += kDepth) {
#pragma unroll
      for (int d = 0; d < kDepth; ++d) {
        const int ki = i0 + d;
        if (ki >= nk) break;
        float* mine = planes[wave];
#pragma unroll
        for (int j = 0; j < PL; ++j) {
            const int piece = lane + 64 * j;
            if (piece < NP) P::widen(pre[d][j], mine + piece * P::kPerPiece);
        }
        if (ki + kDepth < nk) fetch(ki + kDepth, pre[d]);
        __builtin_amdgcn_wave_barrier();                       // wave-private tile: LDS ops of one wave stay in order
        // x pass on row PAIRS (v_pk_fma_f32: two rows per instruction); h2[yp] = (h[2yp], h[2yp+1]).
        // LDS gathers are issued XB row pairs ahead of their use so their latency overlaps.
        float2v h2[S / 2];
        constexpr int XB = 4;
#pragma unroll
        for (int y0 = 0; y0 < S / 2; y0 += XB) {
            float2v t0[XB], t1[XB], t2[XB], t3[XB];
#pragma unroll
            for (int j = 0; j < XB; ++j) {
                const int ra = 2 * (y0 + j) * S, rb = ra + S;
                t0[j] = float2v{x0[ra], x0[rb]};
                t1[j] = float2v{x1[ra], x1[rb]};
                t2[j] = float2v{x2[ra], x2[rb]};
                t3[j] = float2v{x3[ra], x3[rb]};
            }
            __builtin_amdgcn_sched_barrier(0);
            // tap-major: XB independent accumulation chains in flight (a dependent v_pk_fma_f32 cannot
            // issue back-to-back)
            float2v v[XB];
#pragma unroll
            for (int j = 0; j < XB; ++j) v[j] = t0[j] * wx0;
#pragma unroll
            for (int j = 0; j < XB; ++j) v[j] = __builtin_elementwise_fma(t1[j], float2v{wx1, wx1}, v[j]);
#pragma unroll
            for (int j = 0; j < XB; ++j) v[j] = __builtin_elementwise_fma(t2[j], float2v{wx2, wx2}, v[j]);
#pragma unroll
            for (int j = 0; j < XB; ++j) h2[y0 + j] = __builtin_elementwise_fma(t3[j], float2v{wx3, wx3}, v[j]);
        }
        __builtin_amdgcn_wave_barrier();
        // y pass on OUTPUT row pairs that share their 4 source rows (R = 2: (1,2), (3,4), ..., rows 0
        // and 63 alone; R = 4: (0,1), (2,3), ...): each source row is broadcast against the pair of
        // its two coefficients.
        auto hrow = [&](int r) { const int rc = clamp_row<S>(r); return h2[rc >> 1][rc & 1]; };
        if (P0 == 1) {
            const int fa = src_floor<S, O>(0), fb = src_floor<S, O>(O - 1);
            const float* wa = tw + (0 % R) * 4;
            const float* wb = tw + ((O - 1) % R) * 4;
            float va = hrow(fa - 1) * wa[0], vb = hrow(fb - 1) * wb[0];
#pragma unroll
            for (int a = 1; a < 4; ++a) {
                va = __builtin_fmaf(hrow(fa - 1 + a), wa[a], va);
                vb = __builtin_fmaf(hrow(fb - 1 + a), wb[a], vb);
            }
            edge[0] += fmaxf(va, 0.f);
            edge[1] += fmaxf(vb, 0.f);
        }
        constexpr int YB = 8;                                  // independent output pairs in flight
        constexpr int NPAIR = (O - P0) / 2;
#pragma unroll
        for (int p0 = 0; p0 < NPAIR; p0 += YB) {
            float2v v[YB];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int j = 0; j < YB; ++j) {
                    const int p = p0 + j;
                    if (p < NPAIR) {
                        const int o = P0 + 2 * p;
                        const int f = src_floor<S, O>(o);      // == src_floor(o + 1) by construction
                        const float hv = hrow(f - 1 + a);
                        const float2v w = {tw[(o % R) * 4 + a], tw[((o + 1) % R) * 4 + a]};   // uniform: scalar loads
                        v[j] = a == 0 ? float2v{hv, hv} * w : __builtin_elementwise_fma(float2v{hv, hv}, w, v[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < YB; ++j)
                if (p0 + j < NPAIR) acc2[p0 + j] += float2v{fmaxf(v[j][0], 0.f), fmaxf(v[j][1], 0.f)};
        }
      }
    }
    auto get = [&](int oy) -> float {
        if (P0 == 1 && oy == 0) return edge[0];
        if (P0 == 1 && oy == O - 1) return edge[1];
        return acc2[(oy - P0) >> 1][(oy - P0) & 1];
    };
    auto add = [&](int oy, float v) {
        if (P0 == 1 && oy == 0) edge[0] += v;
        else if (P0 == 1 && oy == O - 1) edge[1] += v;
        else acc2[(oy - P0) >> 1][(oy - P0) & 1] += v;
    };
    wg_reduce_flush(red, wave, get, add,
                    [&](int i) { return i * O + lane; }, L.out + (size_t)tok * O * O, L.inv_n);
