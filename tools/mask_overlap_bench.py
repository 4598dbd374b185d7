"""Scoring W masks against G masks of one size: one ``evaluate.mask_overlap_matrix`` call (``daam_mask_overlap_matrix``: the u8 bytes
read once, exact counts) against the route there was before it, ``evaluate.mask_overlap`` on the W x G expanded f32 pairs, in one
process with the legs alternating:

  * ``matrix``  : ``mask_overlap_matrix(a, b)`` on the uint8 stacks -- two launches, counts left on the device;
  * ``pairs``   : ``mask_overlap(a_pairs, b_pairs)`` on f32 stacks of W x G pairs that are already there -- one launch;
  * ``expand``  : making those stacks from the uint8 masks (widen to f32, repeat every mask G or W times), which a user of the pair
                  route has to pay for first.

256^2 and 1024^2 with W = G = 3, 10, 32; 832 x 1216 with W = G = 10; and one stack against itself (``b = None``) at W = 32, where the
pair route has no leg.  Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps, which is what a
caller waits for); the table reports the median and the spread (min, max) of each leg.  ``ratio`` = matrix / pairs medians.
``peak_fraction`` = (n_a + n_b) x h x w bytes over the matrix median over 8 TB/s: only meaningful where the call is not launch overhead.

    python tools/mask_overlap_bench.py [--out profiles/mask_overlap_matrix.json] [--reps 30]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from daam_amd import build, evaluate as EV  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def expand(a, b):
    """[W, h, w] and [G, h, w] uint8 -> two f32 stacks of W x G pairs, pair (i, j) at i * G + j."""
    w, g = a.shape[0], b.shape[0]
    return (a.to(torch.float32).repeat_interleave(g, dim=0), b.to(torch.float32).repeat(w, 1, 1))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_overlap_matrix.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    points = [((s, s), n, False) for s in (256, 1024) for n in (3, 10, 32)] + [((832, 1216), 10, False)] + \
             [((256, 256), 32, True), ((1024, 1024), 32, True)]
    rows = []
    for (h, w), n, one_stack in points:
        a = torch.from_numpy((rng.random((n, h, w)) < 0.3).astype(np.uint8)).cuda()
        b = None if one_stack else torch.from_numpy((rng.random((n, h, w)) < 0.3).astype(np.uint8)).cuda()
        fns = dict(matrix=lambda: EV.mask_overlap_matrix(a, b))
        got = fns['matrix']()
        if not one_stack:
            pa, pb = expand(a, b)
            fns['pairs'] = lambda: EV.mask_overlap(pa, pb)
            fns['expand'] = lambda: expand(a, b)
            sums = fns['pairs']().to(torch.int32).view(n, n, 3)
            same = bool(torch.equal(sums[:, :, 0], got.intersection) and torch.equal(sums[:, 0, 1], got.area_a)
                        and torch.equal(sums[0, :, 2], got.area_b))
        else:
            same = bool(torch.equal(got.intersection, got.intersection.t()) and torch.equal(got.intersection.diagonal(), got.area_a))
        samples = measure(fns, args.reps)
        med = {k: statistics.median(v) for k, v in samples.items()}
        mask_bytes = (n if one_stack else 2 * n) * h * w
        row = dict(size=[h, w], n_a=n, n_b=n, one_stack=one_stack, counts_equal=same,
                   ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                   bytes=dict(matrix=mask_bytes, pairs=None if one_stack else 2 * 4 * n * n * h * w),
                   peak_fraction=round(mask_bytes / (med['matrix'] * 1e-3) / PEAK_BYTES_PER_S, 4))
        if not one_stack:
            row['ratio'] = round(med['matrix'] / med['pairs'], 3)
            row['ratio_with_expand'] = round(med['matrix'] / (med['pairs'] + med['expand']), 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del a, b, fns
        if not one_stack:
            del pa, pb
    res = dict(workload=f'Bernoulli(0.3) uint8 masks; one sample = one call of a leg between two HIP events, legs alternating, '
                        f'{args.reps} samples per leg after 3 warm-up rounds',
               device=torch.cuda.get_device_name(0), kernel_shas={k: v for k, v in build.kernel_shas().items() if 'mask_' in k},
               results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
