// body of finalize_kernel and of its grouped form (daam_finalize_groups); included inside the kernel, where `L` is the launch
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int tok = blockIdx.x;
    const int chunk = blockIdx.y;
    const int O = L.out_side;
    float* outt = reinterpret_cast<float*>(smem_raw);            // [O][O]
    float* plane = outt + O * O;                                 // [max_side][max_side]
    float* tmp = plane + L.max_side * L.max_side;                // [max_side][O]
    const int tid = threadIdx.x;
    for (int i = tid; i < O * O; i += 256) outt[i] = 0.f;

    for (int kidx = chunk; kidx < L.n_keys; kidx += L.n_chunks) {
        const FinKey key = L.keys[kidx];
        const int S = key.side;
        const ACC_T* src = reinterpret_cast<const ACC_T*>(key.base) + (size_t)tok * S * S;
        if (key.tab < 0) {                                       // same size: copy (+ clamp)
            for (int i = tid; i < O * O; i += 256) outt[i] += fmaxf(ld<ACC_T>(src + i), 0.f);
            continue;
        }
        const int16_t* tix = L.tab_idx + (size_t)key.tab * O * 4;
        const float* tw = L.tab_w + (size_t)key.tab * O * 4;
        __syncthreads();                                         // previous key done with plane/tmp
        for (int i = tid; i < S * S; i += 256) plane[i] = ld<ACC_T>(src + i);
        __syncthreads();
        for (int i = tid; i < S * O; i += 256) {
            const int y = i / O, ox = i - y * O;
            const float* row = plane + y * S;
            const int16_t* ix = tix + ox * 4;
            const float* w = tw + ox * 4;
            tmp[i] = row[ix[0]] * w[0] + row[ix[1]] * w[1] + row[ix[2]] * w[2] + row[ix[3]] * w[3];
        }
        __syncthreads();
        for (int i = tid; i < O * O; i += 256) {
            const int oy = i / O, ox = i - oy * O;
            const int16_t* iy = tix + oy * 4;
            const float* w = tw + oy * 4;
            const float v = tmp[iy[0] * O + ox] * w[0] + tmp[iy[1] * O + ox] * w[1] +
                            tmp[iy[2] * O + ox] * w[2] + tmp[iy[3] * O + ox] * w[3];
            outt[i] += fmaxf(v, 0.f);
        }
    }
    // each thread only ever touched its own outt[i] entries (i = tid mod 256): no barrier needed
    float* out = L.out + (size_t)tok * O * O;
    for (int i = tid; i < O * O; i += 256) atomicAdd(out + i, outt[i] * L.inv_n);
