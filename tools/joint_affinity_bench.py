"""The joint affinity (include/daam_joint_affinity.h) at the shapes it is built for -- SD3-medium at 1024 x 1024 (fp16,
24 heads, P = Pk = 4096, d = 64, T = 154) and FLUX.1 at 1024 x 1024 (bf16, 24 heads, d = 128, T = 512), batch 1 -- the HIP path against
a plain torch restatement on the same GPU, in one process with the legs alternating.

  * ``tap``            : (a) ``JointTapState.tap`` of one call onto existing sums -- two launches (statistics, text columns);
  * ``tap_affinity``   : (b) the same followed by ``JointAffinityState.tap`` on its statistics -- a third launch (image columns);
  * ``torch_affinity`` : (c) ``bmm`` over the concatenated keys, ``softmax`` (f32), a slice of the image columns, a sum over heads and
                         ``add_`` -- the yardstick, written plainly and not tuned.  It materialises [heads, P, T + Pk].

Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps); the table reports the median and the
spread of each leg and (b) - (a), the cost of the option, beside the image kernel's floors: the MFMA flops (the image columns once),
the exponentials (one per entry and slice), the bytes of sums (read and written once).  ``max_abs_difference`` compares the two
routes' matrices.  The bar: the median of (b) minus the median of (a) is <= the median of (c).

    python tools/joint_affinity_bench.py [--out profiles/joint_affinity.json] [--reps 20]
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
SHAPES = {'sd3_medium_1024': (torch.float16, 24, 64, 64, 154, 64), 'flux1_1024': (torch.bfloat16, 24, 64, 64, 512, 128)}   # dtype, heads, h, w, T, d


def torch_affinity(q, k_txt, k_img, heads, scale, sums):
    b, p, c = q.shape

    def split(t):
        return t.view(b, t.shape[1], heads, c // heads).permute(0, 2, 1, 3).reshape(b * heads, t.shape[1], c // heads)
    keys = torch.cat([split(k_txt), split(k_img)], dim=1)
    probs = torch.softmax(torch.bmm(split(q), keys.transpose(1, 2)) * scale, dim=-1, dtype=torch.float32)
    sums.add_(probs[:, :, k_txt.shape[1]:].sum(dim=0))
    return sums


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


def bench_shape(name, dtype, heads, h, w, t, d, reps):
    p = h * w
    gen = torch.Generator(device='cuda').manual_seed(5)
    q, k_img = ((0.7 * torch.randn(1, p, heads * d, generator=gen, device='cuda')).to(dtype) for _ in range(2))
    k_txt = (0.7 * torch.randn(1, t, heads * d, generator=gen, device='cuda')).to(dtype)
    scale = d ** -0.5
    state, aff = E.JointTapState(h, w, t), E.JointAffinityState(h, w)

    def both():
        state.tap(q, k_txt, k_img, heads, scale)
        aff.tap(q, k_img, heads, scale, state.stats)
    both()
    theirs = torch_affinity(q, k_txt, k_img, heads, scale, torch.zeros(p, p, device='cuda'))
    difference = float((aff.sums - theirs).abs().max())
    fns = {'tap': lambda: state.tap(q, k_txt, k_img, heads, scale), 'tap_affinity': both,
           'torch_affinity': lambda: torch_affinity(q, k_txt, k_img, heads, scale, theirs)}
    samples = measure(fns, reps)
    med = {leg: statistics.median(v) for leg, v in samples.items()}
    cost = med['tap_affinity'] - med['tap']
    floors = dict(mfma_ms=2 * heads * p * p * d / MFMA_PEAK * 1e3, exp_ms=heads * p * p / EXP_PEAK * 1e3, sums_ms=2 * 4 * p * p / HBM_PEAK * 1e3)
    floor = max(floors.values())
    row = dict(shape=name, dtype=str(dtype).replace('torch.', ''), heads=heads, P=p, T=t, d=d, floors_ms={key: round(v, 4) for key, v in floors.items()},
               ms={key: dict(median=round(med[key], 4), min=round(min(samples[key]), 4), max=round(max(samples[key]), 4)) for key in fns},
               affinity_cost_ms=round(cost, 4), largest_floor_ms=round(floor, 4), cost_over_largest_floor=round(cost / floor, 2),
               speedup=round(med['torch_affinity'] / cost, 2) if cost > 0 else None, bar_met=bool(cost <= med['torch_affinity']),
               max_abs_difference=difference)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_affinity.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rows = [bench_shape(name, *shape, args.reps) for name, shape in SHAPES.items()]
    failed = [r['shape'] for r in rows if not r['bar_met']]
    bar = dict(rule='median(tap_affinity) - median(tap) <= median(torch_affinity)', met=not failed, failed=failed)
    shapes = {name: (str(s[0]).replace('torch.', ''),) + s[1:] for name, s in SHAPES.items()}
    res = dict(workload=f'one joint-attention call, batch 1, shapes {shapes} as (dtype, heads, h, w, T, d), Pk = P = h w; one sample = one call '
                        f'of a leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               yardstick='torch: bmm over the concatenated keys, softmax in f32, a slice of the image columns, a sum over heads, add_; on the same GPU',
               not_measured='the image kernel alone (no kernel trace was taken): its time is read off as tap_affinity - tap, two medians',
               peaks=dict(hbm_bytes_per_s=HBM_PEAK, mfma_fp16_flops_per_s=MFMA_PEAK, exp_per_s=EXP_PEAK), device=torch.cuda.get_device_name(0),
               kernel_shas=dict(jointaff=build.kernel_shas(build.JOINT_AFFINITY_LIB), joint=build.kernel_shas(build.JOINT_LIB)), bar=bar, results=rows)
    print(json.dumps(dict(bar=bar)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
