"""Head analysis at the SDXL-1024 topology: one ``HeatMapEngine.key_scores`` call (``daam_key_scores``: the running sums read once,
no map written) against the only route there was before it, in one process on the same buffers:

  * ``key_scores`` : one call for all 1100 keys x 77 rows x M footprints;
  * ``loop``       : per key ``engine.global_heat_map(head_idx=, layer_idx=)`` then ``engine.region_dots`` (M = 0: the sum of the map);
  * ``finalize``   : ``engine.global_heat_map()`` of the same keys -- it reads the same plane bytes (compared with M = 0).

Synthetic signed fp16 sums: 10 layers x 10 heads x 64^2 and 50 layers x 20 heads x 32^2, 77 rows.  Every sample is one call of a leg
between two HIP events after warm-up rounds, the legs alternating; the table reports median, min and max.  ``peak_fraction`` = plane
bytes over the ``key_scores`` median over 8 TB/s.  ``agree``: both routes within 1e-3 of each other relative to the largest score (a
plausibility check; the bound is held by tests/test_gpu_key_scores.py).

    python tools/key_scores_bench.py [--out profiles/key_scores.json] [--reps 30] [--loop-reps 3]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from daam_amd import _native as nat, build, engine  # noqa: E402
from mask_overlap_bench import measure  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
ROWS = 77
TOPOLOGY = [(64, 10, 1)] * 10 + [(32, 20, 2)] * 50              # (side, heads, factor) per layer


def make_engine():
    eng = engine.HeatMapEngine(len(TOPOLOGY), tokens=ROWS, out_side=64)
    eng.device = torch.device('cuda:0')
    eng._ensure_ctx(torch.float16)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    plane_bytes = 0
    for i, (side, heads, factor) in enumerate(TOPOLOGY):
        eng._ensure_layer(i, heads, side, factor)
        nat.check(eng.lib.daam_layer_touch(eng.ctx, i, eng.stream))
        eng._touch(i)
        acc = eng.acc[i]
        acc.copy_((torch.randn(acc.shape, generator=g, device='cuda:0', dtype=torch.float32) + 0.5).to(acc.dtype))
        plane_bytes += acc.numel() * acc.element_size()
    return eng, plane_bytes


def loop(eng, keys, footprint):
    out = []
    for _, layer, head in keys:
        m = eng.global_heat_map(head_idx=head, layer_idx=layer)
        out.append(m.sum(dim=(1, 2))[None] if footprint is None else engine.region_dots(m, footprint))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'key_scores.json'))
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--loop-reps', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng, plane_bytes = make_engine()
    g = torch.Generator(device='cuda:0').manual_seed(2)
    rows = []
    for n in (0, 1, 8, 32):
        fp = None if n == 0 else (torch.randn(n, 64, 64, generator=g, device='cuda:0') * 0.5 + 0.3).contiguous()
        keys, got = eng.key_scores(fp)
        assert len(keys) == 1100
        want = loop(eng, keys, fp)
        agree = bool(((got - want).abs().max() <= 1e-3 * want.abs().max()).item())
        fast = measure({'key_scores': lambda: eng.key_scores(fp), 'finalize': lambda: eng.global_heat_map()}, args.reps)
        slow = measure({'loop': lambda: loop(eng, keys, fp)}, args.loop_reps, warmup=1)
        samples = dict(fast, **slow)
        med = {k: statistics.median(v) for k, v in samples.items()}
        row = dict(n_masks=n, keys=len(keys), rows=ROWS, agree=agree, plane_bytes=plane_bytes,
                   footprint_bytes_per_batch=n * 64 * 64 * 4,
                   ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4), samples=len(v)) for k, v in samples.items()},
                   peak_fraction=round(plane_bytes / (med['key_scores'] * 1e-3) / PEAK_BYTES_PER_S, 4),
                   speedup_over_loop=round(med['loop'] / med['key_scores'], 1),
                   over_finalize=round(med['key_scores'] / med['finalize'], 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = dict(workload='SDXL-1024 topology, synthetic signed fp16 sums: 10 x 10 x 64^2 + 50 x 20 x 32^2 planes per row, 77 rows, 1100 keys; one '
                        f'sample = one call of a leg between two HIP events; {args.reps} samples (loop: {args.loop_reps}) after warm-up',
               device=torch.cuda.get_device_name(0),
               kernel_shas={k: v for k, v in build.kernel_shas(build.ANALYSIS_OUT).items() if 'key_scores' in k}, results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
