"""The self-attention affinity (include/daam_self_affinity.h) at the two shapes it is built for -- SDXL-1024's own
attn1 of the heat map's grid (10 heads, P = 4096, d = 64, batch 1, fp16) and SD-v1.5's 64 x 64 layer (8 heads, d = 40) -- the HIP path
against a plain torch restatement on the same GPU, in one process with the legs alternating.

  * ``accumulate`` : ``SelfAffinityState.tap`` of one call onto existing sums -- two launches (statistics, sums);
  * ``iteration``  : ``engine.affinity_propagate(sums, maps, 1)`` with N = 8 maps -- the row sums and one iteration;
  * ``torch_*``    : ``bmm``, ``softmax`` (f32), a sum over heads and ``add_``; a ``mm`` and a division -- the yardstick, written plainly and
                     not tuned.  It materialises [heads, P, P].

Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps and the allocation of the outputs);
the table reports the median and the spread of each leg beside the leg's floors: the MFMA flops (Q K^T is computed twice), the
exponentials (one per entry and kernel), the bytes of ``sums`` (read and written once; per iteration read once).
``marginal_iteration`` is (call of 11 - call of 1) / 10: an iteration without the call's fixed costs and the row sums.
``max_abs_difference`` compares the two routes' results.  The bar: every HIP leg's median is <= its torch leg's.

    python tools/self_affinity_bench.py [--out profiles/self_affinity.json] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from daam_amd import build, engine as E  # noqa: E402

HBM_PEAK = 8.0e12                            # bytes per second
MFMA_PEAK = 2.5e15                           # dense fp16 flops per second
EXP_PEAK = 256 * 4 * 16 * 2.4e9              # v_exp_f32 per second: 16 lanes per clock and SIMD
SHAPES = {'sdxl_1024': (10, 4096, 64), 'sd15_512': (8, 4096, 40)}
N_MAPS = 8


def torch_accumulate(q, k, heads, scale, sums):
    b, p, c = q.shape
    qh = q.view(b, p, heads, c // heads).permute(0, 2, 1, 3).reshape(b * heads, p, c // heads)
    kh = k.view(b, p, heads, c // heads).permute(0, 2, 1, 3).reshape(b * heads, p, c // heads)
    sums.add_(torch.softmax(torch.bmm(qh, kh.transpose(1, 2)) * scale, dim=-1, dtype=torch.float32).sum(dim=0))
    return sums


def torch_propagate(sums, maps, iterations):
    n, h, w = maps.shape
    m = maps.reshape(n, h * w)
    total = sums.sum(dim=1)
    for _ in range(iterations):
        m = torch.mm(m, sums.t()) / total
    return m.reshape(n, h, w)


def measure(fns, reps, warmup=3):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {name: [] for name in fns}
    for r in range(warmup + reps):
        for name, fn in fns.items():                        # the legs alternate
            torch.cuda.synchronize()
            start.record()
            fn()
            end.record()
            end.synchronize()
            if r >= warmup:
                samples[name].append(start.elapsed_time(end))
    return samples


def bench_shape(name, heads, p, d, reps):
    side = int(p ** 0.5)
    gen = torch.Generator(device='cuda').manual_seed(5)
    q = (0.7 * torch.randn(1, p, heads * d, generator=gen, device='cuda')).half()
    k = (0.7 * torch.randn(1, p, heads * d, generator=gen, device='cuda')).half()
    maps = torch.rand(N_MAPS, side, side, generator=gen, device='cuda')
    scale = d ** -0.5
    state = E.SelfAffinityState(side, side)
    state.tap(q, k, heads, scale)
    theirs = torch_accumulate(q, k, heads, scale, torch.zeros(p, p, device='cuda'))
    difference = dict(sums=float((state.sums - theirs).abs().max()),
                      propagated=float((E.affinity_propagate(state.sums, maps, 2) - torch_propagate(state.sums, maps, 2)).abs().max()))
    torch_sums = theirs
    fns = {
        'accumulate': lambda: state.tap(q, k, heads, scale), 'torch_accumulate': lambda: torch_accumulate(q, k, heads, scale, torch_sums),
        'iteration': lambda: E.affinity_propagate(state.sums, maps, 1), 'torch_iteration': lambda: torch_propagate(state.sums, maps, 1),
        'call_of_11': lambda: E.affinity_propagate(state.sums, maps, 11), 'call_of_1': lambda: E.affinity_propagate(state.sums, maps, 1),
    }
    samples = measure(fns, reps)
    med = {leg: statistics.median(v) for leg, v in samples.items()}
    dp = -(-d // 16) * 16
    floors = dict(accumulate=dict(mfma_ms=2 * 2 * heads * p * p * dp / MFMA_PEAK * 1e3, exp_ms=2 * heads * p * p / EXP_PEAK * 1e3,
                                  hbm_ms=2 * 4 * p * p / HBM_PEAK * 1e3),
                  iteration=dict(hbm_ms=4 * p * p / HBM_PEAK * 1e3))
    rows, failed = [], []
    for leg in ('accumulate', 'iteration'):
        floor = max(floors[leg].values())
        row = dict(shape=name, leg=leg, floors_ms={key: round(v, 4) for key, v in floors[leg].items()},
                   ms={key: dict(median=round(med[key], 4), min=round(min(samples[key]), 4), max=round(max(samples[key]), 4))
                       for key in (leg, 'torch_' + leg)},
                   fraction_of_floor={key: round(v / med[leg], 4) for key, v in floors[leg].items()}, largest_floor_ms=round(floor, 4),
                   speedup=round(med['torch_' + leg] / med[leg], 2), bar_met=bool(med[leg] <= med['torch_' + leg]))
        if not row['bar_met']:
            failed.append(f'{name}/{leg}')
        print(json.dumps(row), flush=True)
        rows.append(row)
    marginal = (med['call_of_11'] - med['call_of_1']) / 10
    extra = dict(shape=name, marginal_iteration_ms=round(marginal, 4), marginal_fraction_of_hbm_peak=round(4 * p * p / HBM_PEAK * 1e3 / marginal, 4),
                 max_abs_difference=difference)
    print(json.dumps(extra), flush=True)
    return rows, extra, failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'self_affinity.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rows, extras, failed = [], [], []
    for name, (heads, p, d) in SHAPES.items():
        r, x, f = bench_shape(name, heads, p, d, args.reps)
        rows += r
        extras.append(x)
        failed += f
    bar = dict(ratio=1.0, met=not failed, failed=failed)
    res = dict(workload=f'one attn1 call, batch 1, fp16, shapes {SHAPES} as (heads, P, d); propagation of {N_MAPS} maps; one sample = one call of a '
                        f'leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               yardstick='torch: bmm, softmax in f32, a sum over heads, add_; mm and a division; on the same GPU',
               peaks=dict(hbm_bytes_per_s=HBM_PEAK, mfma_fp16_flops_per_s=MFMA_PEAK, exp_per_s=EXP_PEAK), device=torch.cuda.get_device_name(0),
               kernel_shas=build.kernel_shas(build.SELFAFF_LIB), bar=bar, results=rows, marginal=extras)
    print(json.dumps(dict(bar=bar)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
