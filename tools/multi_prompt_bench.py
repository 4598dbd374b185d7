"""Grouped finalize against one finalize per prompt: ``daam_finalize_groups`` (N per-prompt global heat maps, one launch per
class) vs N sequential ``daam_finalize`` calls, on the synthetic SDXL-1024 and SD-v1.5 topologies (tools/synthetic_unet.py), for
N = 1, 2, 4, 8 prompts and the three sums dtypes.  The running sums of a batched generation (kept keys = N x heads per layer)
are filled with random values directly; every prompt's map has all 77 rows.  Prints one JSON document (``--out`` writes it too).
Finalize only: whole generations (maps/s with N prompts per ``pipe()`` call against N single-prompt calls) are not measured here.

    python tools/multi_prompt_bench.py --out profiles/multi_prompt_finalize.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (bench.py)
DTYPES = {'f16': (torch.float16, 'exact'), 'bf16': (torch.bfloat16, 'exact'), 'f32': (torch.float16, 'float32')}


def layers_of(kind):
    """(heads, side, factor) of every tapped cross-attention layer, in execution order (trace.py:285, :289)."""
    from tools.synthetic_unet import SyntheticUNet
    unet = SyntheticUNet(kind, latent=128 if kind == 'sdxl' else 64)
    latent_hw = 4096
    out = []
    for attn, res in unet.attn2_in_execution_order():
        factor = int(math.sqrt(latent_hw // (res * res)))
        if factor != 8:
            out.append((attn.heads, res, factor))
    return out


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ts.append(start.elapsed_time(stop))
    ts.sort()
    return ts[len(ts) // 2]


def run(kind, dt, n, reps):
    from daam_amd import _native as nat
    from daam_amd.engine import HeatMapEngine
    pipe_dtype, accumulate = DTYPES[dt]
    layers = layers_of(kind)
    eng = HeatMapEngine(len(layers), tokens=77, out_side=64, accumulate=accumulate)
    eng.device = torch.device('cuda:0')
    eng._ensure_ctx(pipe_dtype if dt != 'bf16' else torch.bfloat16)
    g = torch.Generator(device='cuda:0').manual_seed(n)
    plane_bytes = 0
    for i, (heads, side, factor) in enumerate(layers):
        eng._ensure_layer(i, n * heads, side, factor)
        nat.check(eng.lib.daam_layer_touch(eng.ctx, i, eng.stream))      # a zeroing still owed goes first
        eng._touch(i)
        acc = eng.acc[i]
        acc.copy_(torch.rand(acc.shape, generator=g, device='cuda:0', dtype=torch.float32).to(acc.dtype))
        plane_bytes += acc.numel() * acc.element_size()
    torch.cuda.synchronize()
    table = eng.key_groups(n)
    total = len(table)
    groups = (ctypes.c_int32 * total)(*table)
    rows = (ctypes.c_int32 * n)(*([77] * n))
    masks = [(ctypes.c_uint8 * total)(*[1 if t == p else 0 for t in table]) for p in range(n)]
    plane = 64 * 64
    out = torch.empty(n, 77, 64, 64, device='cuda:0')
    stream = eng.stream

    def grouped():
        nat.check(eng.lib.daam_finalize_groups(eng.ctx, groups, n, rows, out.data_ptr(), 77 * plane, stream))

    def sequential():
        for p in range(n):
            nat.check(eng.lib.daam_finalize(eng.ctx, masks[p], 77, out[p].data_ptr(), stream))
    t_seq = timed(sequential, reps)
    t_grp = timed(grouped, reps)
    grouped()
    kernels = eng.last_kernels(1)
    moved = plane_bytes + n * 77 * plane * 4
    eng.close()
    return dict(kind=kind, sums=dt, n_prompts=n, keys=total, sequential_ms=round(t_seq, 4), grouped_ms=round(t_grp, 4),
                speedup=round(t_seq / t_grp, 3), grouped_bytes=moved,
                grouped_hbm_frac=round(moved / (t_grp * 1e-3) / (HBM_PEAK_GBS * 1e9), 4), grouped_kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = []
    for kind in ('sdxl', 'sd15'):
        for dt in ('f16', 'bf16', 'f32'):
            for n in (1, 2, 4, 8):
                r = run(kind, dt, n, a.reps)
                print(json.dumps(r), flush=True)
                res.append(r)
    doc = dict(method='median of --reps HIP-event-timed regions (host launch gaps included); sums filled with random values; '
                      '77 rows per prompt; grouped = one daam_finalize_groups call, sequential = N daam_finalize calls',
               device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
