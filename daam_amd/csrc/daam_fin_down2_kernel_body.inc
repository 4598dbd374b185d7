// body of finalize_down2_kernel and of its grouped form (daam_finalize_groups); included inside the kernel, where `L` is the launch
    constexpr int O = 64, S = 128, RB = 16, NB = S / RB;
    using P2 = Pair2<ACC_T>;
    using Raw = typename P2::Raw;
    __shared__ __align__(16) float red[2 * O * O];
    constexpr int kMaxKeysPerWave = 64;
    __shared__ const void* kbase[4][kMaxKeysPerWave];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = blockIdx.x;
    const float* tw = L.tab_w + (size_t)L.keys[0].tab * O * 4;            // one map size per launch; t = 0.5 for every output
    const float w0 = tw[0], w1 = tw[1];
    // border clamp folded into the weights: lane 0's tap at column -1 is its own x0, lane 63's tap at column 128 its own x1
    const float w1a = lane == 0 ? w1 + w0 : w1, w1b = lane == 63 ? w1 + w0 : w1;

    float acc[O];
#pragma unroll
    for (int i = 0; i < O; ++i) acc[i] = 0.f;

    const int stride = gridDim.y * 4;
    const int first = blockIdx.y * 4 + wave;
    const int nk = first < L.n_keys ? min((L.n_keys - first + stride - 1) / stride, kMaxKeysPerWave) : 0;
    if (lane < nk) kbase[wave][lane] = as_global<FinKey>(L.keys)[first + lane * stride].base;
    __builtin_amdgcn_wave_barrier();

    auto row_ptr = [&](int ki) {
        return reinterpret_cast<const ACC_T*>(kbase[wave][ki]) + (size_t)tok * S * S + 2 * lane;
    };
    auto fetch = [&](const ACC_T* src, int b, Raw (&dst)[RB]) {
#pragma unroll
        for (int r = 0; r < RB; ++r) dst[r] = *as_global<Raw>(src + (size_t)(b * RB + r) * S);
    };
    if (nk > 0) {
        Raw buf[2][RB];
        fetch(row_ptr(0), 0, buf[0]);
        for (int ki = 0; ki < nk; ++ki) {
            const ACC_T* src = row_ptr(ki);
            const ACC_T* nxt = row_ptr(min(ki + 1, nk - 1));              // the last key re-reads its first batch (harmless)
            float hw[4] = {0.f, 0.f, 0.f, 0.f};                            // h[row - 3 .. row]
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b + 1 < NB) fetch(src, b + 1, buf[(b + 1) & 1]);
                else fetch(nxt, 0, buf[(b + 1) & 1]);
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int row = b * RB + r;
                    float x0, x1;
                    P2::cvt(buf[b & 1][r], x0, x1);
                    // columns 2ox - 1 / 2ox + 2 = lane - 1's x1 / lane + 1's x0: DPP wave shift right / left by one lane with
                    // bound_ctrl (lanes 0 / 63 receive 0; their clamped border tap sits in w1a / w1b)
                    const float xl = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x1), 0x138, 0xf, 0xf, true));
                    const float xr = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x0), 0x130, 0xf, 0xf, true));
                    const float h = __builtin_fmaf(w1a, x0, __builtin_fmaf(w1b, x1, w0 * (xl + xr)));
                    hw[0] = hw[1]; hw[1] = hw[2]; hw[2] = hw[3]; hw[3] = h;
                    if (row == 0) hw[2] = h;                               // h[-1] := h[0]  (rows above the plane clamp to row 0)
                    if (row >= 2 && (row & 1) == 0) {                      // h[row - 3 .. row] = h[2oy - 1 .. 2oy + 2], oy = row / 2 - 1
                        const float v = __builtin_fmaf(w1, hw[1] + hw[2], w0 * (hw[0] + hw[3]));
                        acc[row / 2 - 1] += fmaxf(v, 0.f);
                    }
                }
            }
            // oy = 63: h[125], h[126], h[127], h[128] := h[127]
            const float v = __builtin_fmaf(w1, hw[2] + hw[3], w0 * (hw[1] + hw[3]));
            acc[O - 1] += fmaxf(v, 0.f);
        }
    }
    auto get = [&](int oy) -> float { return acc[oy]; };
    auto add = [&](int oy, float v) { acc[oy] += v; };
    wg_reduce_flush(red, wave, get, add, [&](int i) { return i * O + lane; }, L.out + (size_t)tok * O * O, L.inv_n);
