"""IoU counts of W word masks against G truth masks at T thresholds: one ``engine.threshold_sweep`` call (four launches, two of them at
image resolution) against the route it replaces, T times ``engine.word_masks`` + ``evaluate.mask_overlap_matrix`` on the same
inputs, in one process with the legs alternating:

  * ``sweep`` : ``engine.threshold_sweep(word_maps, H, W, thresholds, truth)`` -- int32 counts for all thresholds, on the device;
  * ``route`` : per threshold ``word_masks(maps, words, H, W, threshold=t, labels=False)`` then ``mask_overlap_matrix(masks, truth)``,
                the counts left on the device.

64^2 -> 256^2, 64^2 -> 1024^2 and 52 x 76 -> 832 x 1216; W = G in {3, 10, 32}; T in {2, 21, 64} (evenly spaced in [0, 1]).  Every sample
is one call of a leg between two HIP events (so it holds the host's enqueue gaps, which is what a caller waits for); the table reports
the median and the spread (min, max) of each leg.  ``speedup`` = route / sweep medians; ``counts_equal`` says that the two legs
counted the same integers everywhere.  ``growth_with_T`` is, per shape and W, sweep(T = 64) / sweep(T = 2).

    python tools/threshold_sweep_bench.py [--out profiles/threshold_sweep.json] [--reps 30]
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

from daam_amd import build, engine as E, evaluate as ev  # noqa: E402

ROWS = 77
BAR = dict(source=[64, 64], out=[1024, 1024], n=10, n_thr=21, factor=4.0)


def blobs(rng, rows, h, w):
    """Heat-map-like planes: a bump per row on a noisy floor."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((rows, h, w), np.float32)
    for r in range(rows):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.3) * max(h, w)
        out[r] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.05 * np.abs(rng.standard_normal((h, w)))
    return out


def legs(maps, words, word_maps, out_h, out_w, thresholds, truth):
    def sweep():
        return E.threshold_sweep(word_maps, out_h, out_w, thresholds, truth)

    def route():
        out = []
        for t in thresholds:
            _, masks, _ = E.word_masks(maps, words, out_h, out_w, threshold=t, labels=False)
            out.append(ev.mask_overlap_matrix(masks, truth))
        return out
    return dict(sweep=sweep, route=route)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'threshold_sweep.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    sizes = [((64, 64), (256, 256)), ((64, 64), (1024, 1024)), ((52, 76), (832, 1216))]
    rows, growth, bar = [], [], None
    for src, out in sizes:
        maps = torch.from_numpy(blobs(rng, ROWS, *src)).cuda()
        for n in (3, 10, 32):
            words = [[int(i) for i in rng.integers(1, ROWS - 1, size=int(rng.integers(1, 4)))] for _ in range(n)]
            word_maps = E.word_maps(maps, words)
            # truth: the words' own masks at 0.5, shifted by a quarter of the image
            truth = torch.roll(E.word_masks(maps, words, *out, threshold=0.5, labels=False)[1], (out[0] // 4, out[1] // 4), (1, 2)).contiguous()
            by_t = {}
            for n_thr in (2, 21, 64):
                thresholds = [i / (n_thr - 1) for i in range(n_thr)]
                fns = legs(maps, words, word_maps, *out, thresholds, truth)
                pred, inter, area = fns['sweep']()
                ovs = fns['route']()
                same = (torch.equal(pred, torch.stack([o.area_a for o in ovs], 1)) and torch.equal(area, ovs[0].area_b) and
                        torch.equal(inter, torch.stack([o.intersection for o in ovs], 2)))
                samples = measure(fns, args.reps)
                med = {k: statistics.median(v) for k, v in samples.items()}
                by_t[n_thr] = med['sweep']
                row = dict(source=list(src), out=list(out), n_words=n, n_truth=n, n_thr=n_thr, counts_equal=bool(same),
                           ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                           speedup=round(med['route'] / med['sweep'], 2))
                if [list(src), list(out), n, n_thr] == [BAR['source'], BAR['out'], BAR['n'], BAR['n_thr']]:
                    bar = dict(sweep_ms=round(med['sweep'], 4), route_ms=round(med['route'], 4), factor=BAR['factor'],
                               met=bool(med['sweep'] < med['route'] / BAR['factor']))
                print(json.dumps(row), flush=True)
                rows.append(row)
            growth.append(dict(source=list(src), out=list(out), n_words=n, sweep_T64_over_T2=round(by_t[64] / by_t[2], 3)))
    res = dict(workload=f'{ROWS} blob planes, min-max normalised, W words of 1-3 tokens against W truth masks; one sample = one call of a '
                        f'leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               device=torch.cuda.get_device_name(0), kernel_shas=build.kernel_shas(build.EVAL_LIB),
               route_kernel_shas={k: v for k, v in build.kernel_shas().items() if 'word_masks' in k or 'mask_matrix' in k},
               bar=bar, growth_with_T=growth, results=rows)
    print(json.dumps(dict(bar=bar, growth_with_T=growth)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
