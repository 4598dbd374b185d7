"""Masks and a label map for W words: one ``engine.word_masks`` call (three launches) against the path it replaces, W times
``word_heat_map`` + ``expand_word_map(threshold=)`` (three launches per word, an f32 plane at image resolution per word), in one
process with the legs alternating:

  * ``batched``         : ``engine.word_masks(maps, words, H, W, threshold=0.4)`` -- word maps, u8 masks and the u8 label map, on the device;
  * ``sequential``      : per word ``expand_word_map(word_heat_map(maps, idx), H, W, threshold=0.4)``, results left on the device (no labels:
                          the single-word path has none);
  * ``sequential_cpu``  : the same with ``.cpu()`` behind every word, what ``compute_word_heat_map(w).expand_as(image, threshold=)`` does.

W = 1, 4, 10, 32; a 64 x 64 source to 64^2 .. 1024^2 and a 52 x 76 source to 52 x 76 .. 832 x 1216.  Every sample is one call of a leg
between two HIP events (so it holds the host's enqueue gaps, which is what a caller waits for); the table reports the median and the
spread (min, max) of each leg.  ``ratio`` = batched / sequential medians; ``within_spread`` says whether the batched call is no slower
than the sequential path by more than the spread of its own samples.

    python tools/word_masks_bench.py [--out profiles/word_masks.json] [--reps 30]
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
THRESHOLD = 0.4


def legs(maps, words, out_h, out_w):
    def batched():
        return E.word_masks(maps, words, out_h, out_w, threshold=THRESHOLD)

    def sequential():
        return [E.expand_word_map(E.word_heat_map(maps, idx), out_h, out_w, threshold=THRESHOLD) for idx in words]

    def sequential_cpu():
        return [E.expand_word_map(E.word_heat_map(maps, idx), out_h, out_w, threshold=THRESHOLD).cpu() for idx in words]
    return dict(batched=batched, sequential=sequential, sequential_cpu=sequential_cpu)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'word_masks.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    sizes = [((64, 64), (64 << k, 64 << k)) for k in range(5)] + [((52, 76), (52 << k, 76 << k)) for k in range(5)]
    rows = []
    for src, out in sizes:
        maps = torch.from_numpy(np.abs(rng.standard_normal((ROWS,) + src)).astype(np.float32)).cuda()
        for n_words in (1, 4, 10, 32):
            words = [[int(i) for i in rng.integers(1, ROWS - 1, size=int(rng.integers(1, 4)))] for _ in range(n_words)]
            fns = legs(maps, words, *out)
            _, masks, _ = fns['batched']()
            same = all(torch.equal(m != 0, s != 0) for m, s in zip(masks, fns['sequential']()))
            samples = measure(fns, args.reps)
            med = {k: statistics.median(v) for k, v in samples.items()}
            spread = max(samples['batched']) - min(samples['batched'])
            n = out[0] * out[1]
            row = dict(source=list(src), out=list(out), n_words=n_words, masks_equal=same,
                       ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                       ratio=round(med['batched'] / med['sequential'], 3), ratio_cpu=round(med['batched'] / med['sequential_cpu'], 3),
                       within_spread=bool(med['batched'] <= med['sequential'] + spread),
                       bytes_written=dict(batched=(n_words + 1) * n, sequential=n_words * 2 * 4 * n))
            print(json.dumps(row), flush=True)
            rows.append(row)
    res = dict(workload=f'{ROWS} planes, threshold {THRESHOLD}, min-max normalised; one sample = one call of a leg between two HIP events, '
                        f'legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               device=torch.cuda.get_device_name(0), kernel_shas={k: v for k, v in build.kernel_shas().items() if 'word_' in k},
               source_planes='read through L1 / L2 (LDS staging not built)', lane_run=4, results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
