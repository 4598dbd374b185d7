"""Scoring 77 token rows under M masks: one ``engine.region_scores`` call (``daam_region_scores``: the mask bytes read once, no f32
plane at image resolution) against what there was before it, in one process with the legs alternating:

  * ``region``     : ``region_scores(maps, masks)`` -- four launches, scores / area / footprint left on the device;
  * ``expand+sum`` : 77 x ``expand_word_map(maps[t], H, W, absolute=True)`` into device planes, then ``einsum`` with ``masks.float()``;
  * ``dots only``  : ``region_dots(other_maps, footprint)``: a second map set against the kept footprint -- one launch.

256^2, 1024^2 (64^2 maps) and 832 x 1216 (52 x 76 maps) masks with M = 3, 10, 32.  Every sample is one call of a leg between two HIP
events (so it holds the host's enqueue gaps, which is what a caller waits for); the table reports the median and the spread (min, max)
of each leg.  ``ratio`` = region / expand+sum medians.  ``peak_fraction`` = M x H x W bytes over the region median over 8 TB/s.
``within_bound``: the region scores against the float64 oracle of tests/_region_domain.py, inside its bound; ``legs_agree``: the two
legs apart by no more than that bound, the resize bound 8 u S, and 2^-17 S for the f32 einsum, whose summation order is the
library's (an allowance, not a derivation: its measured error is reported as ``einsum_err_over_S``).

    python tools/region_scores_bench.py [--out profiles/region_scores.json] [--reps 30]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _epilogue_domain as ed  # noqa: E402
import _region_domain as rd  # noqa: E402
from daam_amd import build, engine  # noqa: E402
from mask_overlap_bench import measure  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
ROWS = 77


def expand_sum(maps, masks):
    H, W = masks.shape[1:]
    big = torch.stack([engine.expand_word_map(maps[t], H, W, absolute=True) for t in range(maps.shape[0])])
    return torch.einsum('myx,tyx->mt', masks.float(), big)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'region_scores.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    points = [((64, 64), (s, s), n) for s in (256, 1024) for n in (3, 10, 32)] + [((52, 76), (832, 1216), n) for n in (3, 10, 32)]
    rows = []
    for (h, w), (H, W), n in points:
        maps_np = ed.planes('real', ROWS, h, w, seed=7)
        masks_np = (rng.random((n, H, W)) < 0.3).astype(np.uint8)
        maps, other = torch.from_numpy(maps_np).cuda(), torch.from_numpy(ed.planes('real', ROWS, h, w, seed=8)).cuda()
        masks = torch.from_numpy(masks_np).cuda()
        scores, area, footprint = engine.region_scores(maps, masks)
        fns = {'region': lambda: engine.region_scores(maps, masks), 'expand+sum': lambda: expand_sum(maps, masks),
               'dots only': lambda: engine.region_dots(other, footprint)}
        ref = rd.oracle(masks_np, maps_np[None], h, w)
        got = scores.cpu().numpy()[None]
        old = fns['expand+sum']().cpu().numpy().astype(np.float64)[None]
        within = bool(rd.worst(got, ref) <= 1.0 and np.array_equal(area.cpu().numpy(), ref['area']))
        tol = ref['bound'] + ed.K_RESIZE * ref['mag'] + 2.0 ** -17 * ref['mag']
        agree = bool((np.abs(old - got) <= tol).all())
        samples = measure(fns, args.reps)
        med = {k: statistics.median(v) for k, v in samples.items()}
        mask_bytes = n * H * W
        row = dict(map_size=[h, w], mask_size=[H, W], n_masks=n, rows=ROWS, K=ref['K'], within_bound=within, legs_agree=agree,
                   worst_over_bound=round(rd.worst(got, ref), 4), einsum_err_over_S=float(np.max(np.abs(old - ref['want']) / ref['mag'])),
                   ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                   bytes=dict(region=mask_bytes, expand_sum_planes=4 * ROWS * H * W),
                   peak_fraction=round(mask_bytes / (med['region'] * 1e-3) / PEAK_BYTES_PER_S, 4),
                   ratio=round(med['region'] / med['expand+sum'], 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del maps, other, masks, footprint, fns
    res = dict(workload=f'Bernoulli(0.3) uint8 masks, {ROWS} rows of "real" planes; one sample = one call of a leg between two HIP events, '
                        f'legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               device=torch.cuda.get_device_name(0), kernel_shas={k: v for k, v in build.kernel_shas().items() if 'region_' in k},
               results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
