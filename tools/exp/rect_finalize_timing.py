"""One-off (LABNOTES R8.1): HIP-event time of one daam_finalize (daam_profile_last_ms: table upload + output zeroing + kernels)
through the raw C ABI, fp16 sums of random values, all 77 rows:
  * finalize_rect_kernel<f16> on the key set of SDXL at 832 x 1216 -- 52 x 76 map, 100 keys of 52 x 76, 1000 keys of 26 x 38;
  * finalize_kernel<f16> (DAAM_FORCE_GENERIC=1, the any-shape square kernel) on the SDXL-1024 key set -- 64 x 64 map, 100 keys of
    64 x 64, 1000 keys of 32 x 32;
  * the same square key set on its default route, for scale.
    python tools/exp/rect_finalize_timing.py [reps]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from daam_amd import _native as nat

DEV = 'cuda:0'
TOKENS = 77


def timed(lib, out_hw, big, small, reps, env=None):
    """10 layers of 10 keys [big], 50 layers of 20 keys [small] (bench.topology('sdxl', ...)): (kernels, median us, min us)."""
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        ctx = nat.c_void_p()
        nat.check(lib.daam_ctx_create_rect(60, TOKENS, out_hw[0], out_hw[1], 0, nat.byref(ctx)))
    finally:
        for k in (env or {}):
            del os.environ[k]
    g = torch.Generator(device=DEV).manual_seed(1)
    bufs = []
    for layer in range(60):
        heads, (h, w) = (10, big) if layer < 10 else (20, small)
        buf = torch.randn(heads, TOKENS, h, w, generator=g, device=DEV, dtype=torch.float16)
        nat.check(lib.daam_layer_configure_rect(ctx, layer, heads, h, w, out_hw[0] // h, buf.data_ptr()))
        bufs.append(buf)
    out = torch.empty(TOKENS, *out_hw, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    nat.check(lib.daam_profile_enable(ctx, 1))
    us = []
    for r in range(reps + 3):
        nat.check(lib.daam_finalize(ctx, None, 0, out.data_ptr(), stream))
        ms = ctypes.c_float()
        nat.check(lib.daam_profile_last_ms(ctx, 1, ctypes.byref(ms)))
        if r >= 3:
            us.append(ms.value * 1e3)
    name = ctypes.create_string_buffer(256)
    nat.check(lib.daam_last_kernels(ctx, 1, name, len(name)))
    nat.check(lib.daam_profile_enable(ctx, 0))
    torch.cuda.synchronize()
    lib.daam_ctx_destroy(ctx)
    return dict(kernels=name.value.decode(), out_hw=list(out_hw), keys=f'100 x {big} + 1000 x {small}', reps=reps,
                median_us=round(float(np.median(us)), 1), min_us=round(float(np.min(us)), 1), max_us=round(float(np.max(us)), 1))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    lib = nat.load()
    res = [timed(lib, (52, 76), (52, 76), (26, 38), reps),
           timed(lib, (64, 64), (64, 64), (32, 32), reps, env={'DAAM_FORCE_GENERIC': '1'}),
           timed(lib, (64, 64), (64, 64), (32, 32), reps)]
    for r in res:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
