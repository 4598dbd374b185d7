"""Image-guided refinement (include/daam_refine.h) at 1024 x 1024, 8 words, the default six dilations (K = 48) and 10
iterations: the HIP path against a plain torch restatement on the same GPU, in one process with the legs alternating.

  * ``affinity``  : ``engine.refine_affinity(image)`` -- one launch, K H W weights written;
  * ``iteration`` : ``engine.refine_maps(..., iterations=1, masks=False, labels=False)`` -- one launch;
  * ``call``      : ``engine.refine_maps(..., iterations=10)`` with masks and labels -- ten launches;
  * ``torch_*``   : the same three written with clamped index gathers, ``std``, ``softmax`` and a sum over the K shifted copies -- the
                    yardstick, written plainly and not tuned.

Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps and the allocation of the outputs,
which is what a caller waits for); the table reports the median and the spread of each leg beside the leg's ALGORITHMIC bytes --
what the operation has to move once: the image in and the weights out; per iteration the weights and the maps in and the maps out;
masks and labels out -- and that as a fraction of the HBM peak (8.0 TB/s).  ``marginal_iteration`` is (call of 20 - call of 10) / 10
without masks: an iteration without the call's fixed costs.  ``max_abs_difference`` compares the two routes' results.  The bar:
every HIP leg's median is <= its torch leg's.

    python tools/refine_bench.py [--out profiles/refine.json] [--reps 20]
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

HBM_PEAK = 8.0e12                            # bytes per second
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def scene(rng, h, w):
    """A generated-image-like scene: a few flat regions with soft noise, uint8 [h, w, 3]."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 3), 90.0)
    for _ in range(6):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.3) * h, rng.uniform(0.05, 0.3) * w
        img[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = rng.uniform(20, 235, 3)
    return np.clip(np.rint(img + rng.normal(0, 6, img.shape)), 0, 255).astype(np.uint8)


def soft_maps(rng, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([np.exp(-((yy - rng.uniform(0, h)) ** 2 + (xx - rng.uniform(0, w)) ** 2) / (2 * (0.15 * h) ** 2)) for _ in range(n)]).astype(np.float32)


def shifts(h, w, dilations, device):
    ys, xs = torch.arange(h, device=device), torch.arange(w, device=device)
    return [((ys + dy * d).clamp(0, h - 1), (xs + dx * d).clamp(0, w - 1)) for d in dilations for dy, dx in OFFSETS]


def torch_affinity(image, dilations, scale):
    v = image.permute(2, 0, 1).float() / 255                                        # [C, H, W]
    near = torch.stack([v[:, qy][:, :, qx] for qy, qx in shifts(v.shape[1], v.shape[2], dilations, v.device)])      # [K, C, H, W]
    sigma = torch.cat([near, v[None]]).std(dim=0, unbiased=False)
    return torch.softmax(-((near - v[None]).abs() / (1e-8 + scale * sigma)[None]).mean(dim=1), dim=0)


def torch_apply(weights, dilations, maps, iterations, threshold=None):
    sh = shifts(maps.shape[1], maps.shape[2], dilations, maps.device)
    for _ in range(iterations):
        acc = torch.zeros_like(maps)
        for k, (qy, qx) in enumerate(sh):
            acc += weights[k] * maps[:, qy][:, :, qx]
        maps = acc
    if threshold is None:
        return maps, None, None
    top, owner = maps.max(dim=0)
    return maps, (maps > threshold).to(torch.uint8), torch.where(top > threshold, owner, 255).to(torch.uint8)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--words', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rng = np.random.default_rng(11)
    h = w = args.size
    n, dil, t, thr, scale = args.words, E.REFINE_DILATIONS, 10, 0.4, 0.1
    k = 8 * len(dil)
    image = torch.from_numpy(scene(rng, h, w)).cuda()
    maps = torch.from_numpy(soft_maps(rng, n, h, w)).cuda()
    weights = E.refine_affinity(image, dil, scale)
    per_iteration = 4 * k * h * w + 2 * 4 * n * h * w
    algorithmic = dict(affinity=3 * h * w + 4 * k * h * w, iteration=per_iteration, call=t * per_iteration + n * h * w + h * w)

    fns = {
        'affinity': lambda: E.refine_affinity(image, dil, scale), 'torch_affinity': lambda: torch_affinity(image, dil, scale),
        'iteration': lambda: E.refine_maps(weights, dil, maps, 1, thr, masks=False, labels=False),
        'torch_iteration': lambda: torch_apply(weights, dil, maps, 1),
        'call': lambda: E.refine_maps(weights, dil, maps, t, thr), 'torch_call': lambda: torch_apply(weights, dil, maps, t, thr),
        'call_of_20_plain': lambda: E.refine_maps(weights, dil, maps, 2 * t, thr, masks=False, labels=False),
        'call_of_10_plain': lambda: E.refine_maps(weights, dil, maps, t, thr, masks=False, labels=False),
    }
    theirs_w = fns['torch_affinity']()
    ours, theirs = fns['call'](), torch_apply(weights, dil, maps, t, thr)
    difference = dict(weights=float((weights - theirs_w).abs().max()), refined=float((ours[0] - theirs[0]).abs().max()),
                      mask_pixels=int((ours[1] != theirs[1]).sum()), label_pixels=int((ours[2] != theirs[2]).sum()))
    del theirs_w, ours, theirs
    samples = measure(fns, args.reps)
    med = {name: statistics.median(v) for name, v in samples.items()}
    rows, failed = [], []
    for leg in ('affinity', 'iteration', 'call'):
        floor_ms = algorithmic[leg] / HBM_PEAK * 1e3
        row = dict(leg=leg, algorithmic_bytes=algorithmic[leg], hbm_floor_ms=round(floor_ms, 4),
                   ms={name: dict(median=round(med[name], 4), min=round(min(samples[name]), 4), max=round(max(samples[name]), 4))
                       for name in (leg, 'torch_' + leg)},
                   fraction_of_hbm_peak=round(floor_ms / med[leg], 4), speedup=round(med['torch_' + leg] / med[leg], 2),
                   bar_met=bool(med[leg] <= med['torch_' + leg]))
        if not row['bar_met']:
            failed.append(leg)
        print(json.dumps(row), flush=True)
        rows.append(row)
    marginal = (med['call_of_20_plain'] - med['call_of_10_plain']) / t
    extra = dict(marginal_iteration_ms=round(marginal, 4), marginal_fraction_of_hbm_peak=round(per_iteration / HBM_PEAK * 1e3 / marginal, 4))
    bar = dict(ratio=1.0, met=not failed, failed=failed)
    res = dict(workload=f'{h} x {w} RGB scene, {n} soft maps, dilations {list(dil)} (K = {k}), {t} iterations, threshold {thr}; one sample = one '
                        f'call of a leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               yardstick='torch: clamped index gathers, std, softmax, a sum over K shifted copies, on the same GPU',
               hbm_peak_bytes_per_s=HBM_PEAK, device=torch.cuda.get_device_name(0), kernel_shas=build.kernel_shas(build.REFINE_LIB), bar=bar,
               max_abs_difference=difference, results=rows, **extra)
    print(json.dumps(dict(bar=bar, max_abs_difference=difference, **extra)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
