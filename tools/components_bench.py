"""Connected components of M masks -- labels, counts, the first 256 components' areas and boxes, the largest one: one
``engine.mask_components`` call (seven launches) against the route it replaces on the same buffers, in one process with the legs
alternating:

  * ``components`` : ``engine.mask_components(masks, connectivity=8, max_components=256)`` -- every result on the device;
  * ``route``      : what a user does today.  With scipy: the masks copied to the host, per mask ``scipy.ndimage.label`` (3 x 3
                     structure) and ``find_objects``.  Without scipy: a torch loop on the device that spreads the lowest pixel index
                     of a blob by 3 x 3 max-pooling until nothing changes (checked every 16 rounds), then ``unique``.  The route is
                     written plainly and is not tuned.

Masks: ``blobs`` -- what ``GlobalHeatMap``-like planes give at threshold 0.4 (``engine.word_masks`` on synthetic planes of a bump on a
noisy floor) -- and ``speckle`` -- the same with 1 % of the pixels flipped.  M in {3, 32} at 256^2, 1024^2 and 832 x 1216.  Every sample
is one call of a leg between two HIP events (so it holds the host's enqueue gaps and, for the route, the copy and the host's work,
which is what a caller waits for); the table reports the median and the spread (min, max) of each leg.  ``results_equal`` says that
the two legs gave the same labels, counts and boxes everywhere.  The bar: at every point the call's median is <= the route's
(``bar.met``; ``bar.failed`` lists the points that miss it).

    python tools/components_bench.py [--out profiles/components.json] [--reps 30]
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

try:
    from scipy import ndimage
except ImportError:                                            # the route then stays on the device
    ndimage = None

ROWS = 77
LISTED = 256


def planes(rng, rows, h, w):
    """Heat-map-like planes: a bump or two per row on a noisy floor."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((rows, h, w), np.float32)
    for r in range(rows):
        out[r] = 0.05 * np.abs(rng.standard_normal((h, w)))
        for _ in range(int(rng.integers(1, 3))):
            cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * max(h, w)
            out[r] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return out


def route_scipy(masks):
    """(labels int32 [M, H, W] with -1 on background, counts [M], boxes: per mask int32 [k <= 256, 4]) on the host."""
    host = masks.cpu().numpy()
    structure = np.ones((3, 3), bool)
    labels, counts, boxes = np.empty(host.shape, np.int32), [], []
    for m, mask in enumerate(host):
        lab, k = ndimage.label(mask, structure)
        labels[m] = lab - 1
        counts.append(k)
        boxes.append(np.array([[s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1] for s in ndimage.find_objects(lab)[:LISTED]],
                              np.int32).reshape(-1, 4))
    return labels, counts, boxes


def route_torch(masks):
    """The device route: every set pixel holds N - index, 3 x 3 max-pooling spreads the largest (the lowest index) inside a blob until a
    fixed point; the distinct values in descending order are the components by rank."""
    m, h, w = masks.shape
    on = masks != 0
    seed = (h * w - torch.arange(h * w, device=masks.device, dtype=torch.float32)).reshape(1, h, w)   # exact below 2^24 pixels
    lab = torch.where(on, seed, torch.zeros_like(seed))
    while True:
        prev = lab
        for _ in range(16):
            lab = torch.where(on, torch.nn.functional.max_pool2d(lab[:, None], 3, 1, 1)[:, 0], lab)
        if torch.equal(lab, prev):
            break
    labels, counts, boxes = torch.full((m, h, w), -1, dtype=torch.int32, device=masks.device), [], []
    ys, xs = torch.arange(h, device=masks.device)[:, None].expand(h, w), torch.arange(w, device=masks.device)[None].expand(h, w)
    for i in range(m):
        values, inverse = torch.unique(-lab[i][on[i]], return_inverse=True)
        labels[i][on[i]] = inverse.to(torch.int32)
        counts.append(len(values))
        k = min(len(values), LISTED)
        box = torch.stack([torch.full((k,), w, device=masks.device), torch.full((k,), h, device=masks.device),
                           torch.full((k,), -1, device=masks.device), torch.full((k,), -1, device=masks.device)], 1)
        keep = inverse < k
        y, x, idx = ys[on[i]][keep], xs[on[i]][keep], inverse[keep]
        box[:, 0].scatter_reduce_(0, idx, x, 'amin')
        box[:, 1].scatter_reduce_(0, idx, y, 'amin')
        box[:, 2].scatter_reduce_(0, idx, x, 'amax')
        box[:, 3].scatter_reduce_(0, idx, y, 'amax')
        boxes.append(box.to(torch.int32).cpu().numpy())
    return labels.cpu().numpy(), counts, boxes


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'components.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(3)
    route = route_scipy if ndimage is not None else route_torch
    sizes = [((64, 64), (256, 256)), ((64, 64), (1024, 1024)), ((52, 76), (832, 1216))]
    rows, failed = [], []
    for src, out in sizes:
        maps = torch.from_numpy(planes(rng, ROWS, *src)).cuda()
        for n in (3, 32):
            words = [[int(i) for i in rng.integers(1, ROWS - 1, size=int(rng.integers(1, 4)))] for _ in range(n)]
            blob = E.word_masks(maps, words, *out, threshold=0.4, labels=False)[1]
            flip = torch.from_numpy((rng.random((n,) + out) < 0.01).astype(np.uint8)).cuda()
            for kind, masks in (('blobs', blob), ('speckle', (blob ^ flip).contiguous())):
                fns = dict(components=lambda: E.mask_components(masks, connectivity=8, max_components=LISTED), route=lambda: route(masks))
                labels, counts, comps = (t.cpu().numpy() for t in fns['components']()[:3])
                want = fns['route']()
                same = bool(np.array_equal(labels, want[0]) and counts[:, 0].tolist() == list(want[1]) and
                            all(np.array_equal(comps[m, :len(b), 2:], b) for m, b in enumerate(want[2])))
                samples = measure(fns, args.reps)
                med = {k: statistics.median(v) for k, v in samples.items()}
                met = bool(med['components'] <= med['route'])
                row = dict(out=list(out), n_masks=n, kind=kind, components_per_mask=[int(counts[:, 0].min()), int(counts[:, 0].max())],
                           results_equal=same, ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in samples.items()},
                           speedup=round(med['route'] / med['components'], 2), bar_met=met)
                if not met:
                    failed.append(dict(out=list(out), n_masks=n, kind=kind))
                print(json.dumps(row), flush=True)
                rows.append(row)
    bar = dict(ratio=1.0, met=not failed, failed=failed)
    res = dict(workload=f'M masks of W words of 1-3 tokens at threshold 0.4 ({ROWS} bump planes), plain and with 1 % of the pixels flipped; one '
                        f'sample = one call of a leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               route='scipy.ndimage.label + find_objects after a copy to the host' if ndimage is not None else 'torch max-pool propagation on the device',
               device=torch.cuda.get_device_name(0), kernel_shas=build.kernel_shas(build.COMPONENTS_LIB), bar=bar,
               results_equal=all(r['results_equal'] for r in rows), results=rows)
    print(json.dumps(dict(bar=bar, results_equal=res['results_equal'], route=res['route'])), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
