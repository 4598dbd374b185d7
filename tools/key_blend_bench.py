"""Heat maps of weighted key sets: one ``HeatMapEngine.key_blend`` call (``daam_key_blend``: the running sums of the weighed keys read
once for up to 8 sets) against the only route there was before it, in one process on the same buffers:

  * ``key_blend`` : one call for the whole weight table;
  * ``loop``      : per distinct key of non-zero weight ``engine.global_heat_map(head_idx=, layer_idx=)``, added into the sets' maps
                    with a weighted ``torch`` add;
  * ``finalize``  : ``engine.global_heat_map()`` of every key -- the all-keys leg reads the same plane bytes (reported, not gated).

Legs: every key in one set at 1 / K; 10 keys in one set; 8 sets of 10 disjoint keys.  Topologies: SDXL-1024 (10 x 10 x 64^2 +
50 x 20 x 32^2 planes per row, 1100 keys) and SD-v1.5 (16 layers x 8 heads, sides 64 / 32 / 16 / 8, 128 keys), synthetic signed fp16
sums, 77 rows.  Every sample is one call of a leg between two HIP events (host enqueue included) after warm-up rounds, the legs
alternating; the table reports median, min and max.  ``within``: key_blend's median <= 1.03 x the loop's.  ``peak_fraction`` (all-keys
leg) = plane bytes over the ``key_blend`` median over 8 TB/s.  ``agree``: both routes within 1e-3 of each other relative to the
largest element (a plausibility check; the bound is held by tests/test_gpu_key_blend.py).

    python tools/key_blend_bench.py [--out profiles/key_blend.json] [--reps 30]
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
MARGIN = 1.03
TOPOLOGIES = {                                                   # (side, heads, factor) per layer
    'sdxl-1024': [(64, 10, 1)] * 10 + [(32, 20, 2)] * 50,
    'sd-v1.5': [(64, 8, 1)] * 2 + [(32, 8, 2)] * 2 + [(16, 8, 4)] * 2 + [(8, 8, 8)] + [(16, 8, 4)] * 3 + [(32, 8, 2)] * 3 + [(64, 8, 1)] * 3,
}


def make_engine(topology):
    eng = engine.HeatMapEngine(len(topology), tokens=ROWS, out_side=64)
    eng.device = torch.device('cuda:0')
    eng._ensure_ctx(torch.float16)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    plane_bytes = 0
    for i, (side, heads, factor) in enumerate(topology):
        eng._ensure_layer(i, heads, side, factor)
        nat.check(eng.lib.daam_layer_touch(eng.ctx, i, eng.stream))
        eng._touch(i)
        acc = eng.acc[i]
        acc.copy_((torch.randn(acc.shape, generator=g, device='cuda:0', dtype=torch.float32) + 0.5).to(acc.dtype))
        plane_bytes += acc.numel() * acc.element_size()
    return eng, plane_bytes


def loop(eng, keys, table):
    """``table`` [G, K] on the host: one finalize per key some set weighs, a weighted add per set that weighs it."""
    out = torch.zeros(table.shape[0], ROWS, eng.out_h, eng.out_w, dtype=torch.float32, device=eng.device)
    for k in torch.nonzero(table.abs().sum(dim=0)).flatten().tolist():
        _, layer, head = keys[k]
        m = eng.global_heat_map(head_idx=head, layer_idx=layer)
        for g in torch.nonzero(table[:, k]).flatten().tolist():
            out[g].add_(m, alpha=float(table[g, k]))
    return out


def legs(n_keys):
    every = torch.full((1, n_keys), 1.0 / n_keys)
    g = torch.Generator().manual_seed(4)
    picks = torch.randperm(n_keys, generator=g)[:80].reshape(8, 10)
    ten = torch.zeros(1, n_keys)
    ten[0, picks[0]] = torch.linspace(-1.0, 1.0, 10) + 0.05
    eight = torch.zeros(8, n_keys)
    for s in range(8):
        eight[s, picks[s]] = 0.1
    return {'all keys, 1 set': every, '10 keys, 1 set': ten, '8 sets of 10 disjoint keys': eight}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'key_blend.json'))
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rows = []
    for name, topology in TOPOLOGIES.items():
        eng, plane_bytes = make_engine(topology)
        keys, _ = eng.key_scores()
        for leg, table in legs(len(keys)).items():
            dev = table.to('cuda:0')
            _, got = eng.key_blend(dev)
            want = loop(eng, keys, table)
            agree = bool(((got - want).abs().max() <= 1e-3 * want.abs().max()).item())
            fns = {'key_blend': lambda: eng.key_blend(dev), 'loop': lambda: loop(eng, keys, table)}
            if leg.startswith('all'):
                fns['finalize'] = lambda: eng.global_heat_map()
            samples = measure(fns, args.reps)
            med = {k: statistics.median(v) for k, v in samples.items()}
            row = dict(topology=name, leg=leg, keys=len(keys), distinct_keys=int((table.abs().sum(dim=0) != 0).sum()), sets=table.shape[0],
                       rows=ROWS, agree=agree,
                       ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4), samples=len(v)) for k, v in samples.items()},
                       speedup_over_loop=round(med['loop'] / med['key_blend'], 1), within=bool(med['key_blend'] <= MARGIN * med['loop']))
            if 'finalize' in med:
                row.update(plane_bytes=plane_bytes, over_finalize=round(med['key_blend'] / med['finalize'], 2),
                           peak_fraction=round(plane_bytes / (med['key_blend'] * 1e-3) / PEAK_BYTES_PER_S, 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
        eng.close()
    res = dict(workload=f'synthetic signed fp16 sums, 77 rows, maps of 64 x 64; one sample = one call of a leg between two HIP events, host '
                        f'enqueue included; {args.reps} samples after warm-up, the legs alternating in one process on the same buffers',
               device=torch.cuda.get_device_name(0), margin=MARGIN,
               kernel_shas={k: v for k, v in build.kernel_shas(build.ANALYSIS_OUT).items() if 'key_blend' in k}, results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
