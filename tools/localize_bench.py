"""Boxes of W word masks at T thresholds, the words' peaks, the boxes of G = W truth masks and the pointing hits: one
``engine.localize`` call (four launches, one of them at image resolution per plane kind) against the route it replaces on the same
buffers, in one process with the legs alternating:

  * ``localize`` : ``engine.localize(word_maps, H, W, thresholds, truth)`` -- every result on the device;
  * ``route``    : per threshold ``word_masks(maps, words, H, W, threshold=t, labels=False)`` and the torch reductions that give the
                   masks' boxes (``any`` over rows and columns, first / last index); once per word
                   ``expand_word_map(plane, H, W, absolute=True)`` and ``argmax``; the same torch reductions on the truth masks and
                   one gather for the hits.  The route is written plainly and is not tuned.

64^2 -> 256^2, 64^2 -> 1024^2 and 52 x 76 -> 832 x 1216; W = G in {3, 10, 32}; T in {1, 21} (evenly spaced in [0, 1]; T = 1: 0.4).
Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps, which is what a caller waits for); the
table reports the median and the spread (min, max) of each leg.  ``results_equal`` says that the two legs gave the same integers
everywhere.  The bar: at every point the call's median is <= 1.03 x the route's (``bar.met``; ``bar.failed`` lists the points that
miss it).  ``growth_with_T`` is, per shape and W, localize(T = 21) / localize(T = 1): reported, not gated.

    python tools/localize_bench.py [--out profiles/localize.json] [--reps 30]
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

from daam_amd import build, engine as E  # noqa: E402

ROWS = 77
BAR_RATIO = 1.03


def blobs(rng, rows, h, w):
    """Heat-map-like planes: a bump per row on a noisy floor."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((rows, h, w), np.float32)
    for r in range(rows):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.3) * max(h, w)
        out[r] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.05 * np.abs(rng.standard_normal((h, w)))
    return out


def torch_boxes(masks):
    """int32 [M, 4] x0 y0 x1 y1 of u8 masks [M, H, W], (W, H, -1, -1) when empty: plain torch reductions."""
    m = masks != 0
    h, w = m.shape[1:]
    rows, cols = m.any(2), m.any(1)
    ys, xs = torch.arange(h, device=m.device), torch.arange(w, device=m.device)
    return torch.stack([torch.where(cols, xs, w).amin(1), torch.where(rows, ys, h).amin(1),
                        torch.where(cols, xs, -1).amax(1), torch.where(rows, ys, -1).amax(1)], 1).to(torch.int32)


def legs(maps, words, word_maps, out_h, out_w, thresholds, truth):
    def localize():
        return E.localize(word_maps, out_h, out_w, thresholds, truth)

    def route():
        boxes = []
        for t in thresholds:
            _, masks, _ = E.word_masks(maps, words, out_h, out_w, threshold=t, labels=False)
            boxes.append(torch_boxes(masks))
        at = torch.stack([E.expand_word_map(plane, out_h, out_w, absolute=True).argmax() for plane in word_maps])
        peaks = torch.stack([at % out_w, at // out_w], 1).to(torch.int32)
        return torch.stack(boxes, 1), peaks, torch_boxes(truth), (truth.reshape(truth.shape[0], -1)[:, at] != 0).t()
    return dict(localize=localize, route=route)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'localize.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    sizes = [((64, 64), (256, 256)), ((64, 64), (1024, 1024)), ((52, 76), (832, 1216))]
    rows, growth, failed = [], [], []
    for src, out in sizes:
        maps = torch.from_numpy(blobs(rng, ROWS, *src)).cuda()
        for n in (3, 10, 32):
            words = [[int(i) for i in rng.integers(1, ROWS - 1, size=int(rng.integers(1, 4)))] for _ in range(n)]
            word_maps = E.word_maps(maps, words)
            # truth: the words' own masks at 0.5, shifted by a quarter of the image
            truth = torch.roll(E.word_masks(maps, words, *out, threshold=0.5, labels=False)[1], (out[0] // 4, out[1] // 4), (1, 2)).contiguous()
            by_t = {}
            for n_thr in (1, 21):
                thresholds = [0.4] if n_thr == 1 else [i / (n_thr - 1) for i in range(n_thr)]
                fns = legs(maps, words, word_maps, *out, thresholds, truth)
                boxes, peaks, _, truth_boxes, hits = fns['localize']()
                want = fns['route']()
                same = (torch.equal(boxes, want[0]) and torch.equal(peaks, want[1]) and torch.equal(truth_boxes, want[2]) and
                        torch.equal(hits, want[3]))
                samples = measure(fns, args.reps)
                med = {k: statistics.median(v) for k, v in samples.items()}
                by_t[n_thr] = med['localize']
                met = bool(med['localize'] <= BAR_RATIO * med['route'])
                row = dict(source=list(src), out=list(out), n_words=n, n_truth=n, n_thr=n_thr, results_equal=bool(same),
                           ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                           speedup=round(med['route'] / med['localize'], 2), bar_met=met)
                if not met:
                    failed.append(dict(source=list(src), out=list(out), n_words=n, n_thr=n_thr))
                print(json.dumps(row), flush=True)
                rows.append(row)
            growth.append(dict(source=list(src), out=list(out), n_words=n, localize_T21_over_T1=round(by_t[21] / by_t[1], 3)))
    bar = dict(ratio=BAR_RATIO, met=not failed, failed=failed)
    res = dict(workload=f'{ROWS} blob planes, min-max normalised, W words of 1-3 tokens against W truth masks; one sample = one call of a '
                        f'leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               device=torch.cuda.get_device_name(0), kernel_shas=build.kernel_shas(build.LOCATE_LIB),
               route_kernel_shas={k: v for k, v in build.kernel_shas().items() if 'word_masks' in k or 'word_expand' in k},
               bar=bar, results_equal=all(r['results_equal'] for r in rows), growth_with_T=growth, results=rows)
    print(json.dumps(dict(bar=bar, results_equal=res['results_equal'], growth_with_T=growth)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
