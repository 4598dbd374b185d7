// Body of word_expand_kernel / word_expand_rect_kernel (daam_epilogue.hip): one thread per output pixel of the bicubic resize of a
// word map [SRC_H][SRC_W] (<= 128x128 f32, L1/L2 resident) to [out_h][out_w], and the min / max of the result.  The including kernel
// defines SRC_H and SRC_W (the square kernel: both its `side`) and has word_map, out, out_h, out_w and minmax as parameters.
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    const bool valid = i < out_h * out_w;
    if (valid) {
        const int oy = i / out_w, ox = i - oy * out_w;
        float wy[4], wx[4];
        int iy[4], ix[4];
        {
            const int first = cubic_taps((float)SRC_H / (float)out_h, oy, wy);
            for (int a = 0; a < 4; ++a) iy[a] = min(max(first + a, 0), SRC_H - 1);
        }
        {
            const int first = cubic_taps((float)SRC_W / (float)out_w, ox, wx);
            for (int a = 0; a < 4; ++a) ix[a] = min(max(first + a, 0), SRC_W - 1);
        }
        if (SRC_H == out_h && SRC_W == out_w) {
            v = word_map[i];
        } else {
            float rows[4];
            for (int a = 0; a < 4; ++a) rows[a] = cubic_row(word_map + iy[a] * SRC_W, ix, wx);
            v = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
        }
        store_for_host(out + i, v);
    }
    // wave64 min / max, one atomic pair per wave
    float lo = valid ? v : INFINITY, hi = valid ? v : -INFINITY;
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(reinterpret_cast<int*>(minmax), enc_ordered(lo));
        atomicMax(reinterpret_cast<int*>(minmax) + 1, enc_ordered(hi));
    }
