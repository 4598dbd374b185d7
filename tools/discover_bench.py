"""Discovery (include/daam_discover.h) at the sizes it is built for: the symmetric-KL kernel at A = 256 anchors against
B = 4096 maps of N = 4096 cells (the 64 x 64 grid of SDXL, SD3 and FLUX at 1024 x 1024) and at A = B = 256 (a round of proposals
against themselves), and the whole ``SelfAffinity.discover`` call -- the HIP path against a plain torch restatement on the same GPU,
in one process with the legs alternating.

  * ``pair_kl``       : ``engine.discover_pair_kl`` into an existing matrix -- one launch;
  * ``torch_pair_kl`` : ``0.5 * ((pa[:, None] - pb[None]) * (la[:, None] - lb[None])).sum(-1)``, chunked over A so that [chunk, B, N]
                        f32 takes at most 1 GiB -- the yardstick, written plainly and not tuned;
  * ``discover``      : ``SelfAffinity.discover(anchors=16, threshold, iterations=3, size=(1024, 1024))`` on a block-structured affinity;
  * ``torch_discover``: the same loop with torch in place of the four passes (row sums, log, the chunked KL, ``member @ P`` means,
                        ``F.interpolate`` + ``argmax``).

Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps and, for ``discover``, the two copies
of D to the host); the table reports the median and the spread of each leg beside the kernel's floors: the VALU work (two subtractions
and one fma per (anchor, map, cell) triple at 128 lanes per clock and CU) and the bytes (the four operands read once, D written
once).  The bar: every HIP leg's median is <= its torch leg's.

    python tools/discover_bench.py [--out profiles/discover.json] [--reps 20]
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

from daam_amd import SelfAffinity, build, engine as E  # noqa: E402

HBM_PEAK = 8.0e12                            # bytes per second
VALU_PEAK = 256 * 4 * 32 * 2.4e9             # f32 VALU lane-operations per second: 32 lanes per clock and SIMD
SHAPES = {'anchors_vs_cells': (256, 4096, 4096), 'proposals_vs_proposals': (256, 256, 4096)}      # A, B, N
CHUNK_BYTES = 1 << 30


def torch_pair_kl(pa, la, pb, lb, out):
    step = max(1, CHUNK_BYTES // (4 * pb.shape[0] * pb.shape[1]))
    for a in range(0, pa.shape[0], step):
        out[a:a + step] = 0.5 * ((pa[a:a + step, None] - pb[None]) * (la[a:a + step, None] - lb[None])).sum(-1)
    return out


def torch_prepare(src):
    s = src.sum(dim=1, keepdim=True)
    p = torch.where((s != 0) & torch.isfinite(s), src / s, torch.zeros_like(src))
    return p, torch.log(p.clamp_min(2.0 ** -120))


def torch_discover(aff, anchors, threshold, iterations, size):
    from daam_amd.heatmap import discover_anchors, discover_groups
    h, w = aff.grid
    p, l = torch_prepare(aff.sums)
    idx = torch.as_tensor(discover_anchors(aff.grid, anchors), device=p.device)
    d = torch_pair_kl(p[idx], l[idx], p, l, torch.empty(len(idx), p.shape[0], device=p.device))
    member = d < threshold
    member[torch.arange(len(idx), device=p.device), idx] = True
    props = (member.float() @ p) / member.sum(dim=1, keepdim=True)
    for _ in range(iterations - 1):
        pp, lp = torch_prepare(props)
        groups = discover_groups(torch_pair_kl(pp, lp, pp, lp, torch.empty(len(pp), len(pp), device=p.device)).cpu(), threshold)
        member = torch.zeros(len(groups), len(pp))
        for k, g in enumerate(groups):
            member[k, g] = 1
        member = member.to(p.device)
        props = (member @ pp) / member.sum(dim=1, keepdim=True)
    big = torch.nn.functional.interpolate(props.view(1, -1, h, w), size=size, mode='bilinear', align_corners=False)[0]
    return big.argmax(dim=0).to(torch.uint8), props


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


def _ms(samples):
    return {key: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for key, v in samples.items()}


def bench_pair_kl(name, a, b, n, reps):
    gen = torch.Generator(device='cuda').manual_seed(5)
    pa, la = E.discover_prepare(torch.rand(a, n, generator=gen, device='cuda') + 0.1)
    pb, lb = E.discover_prepare(torch.rand(b, n, generator=gen, device='cuda') + 0.1)
    ours, theirs = E.discover_pair_kl(pa, la, pb, lb), torch_pair_kl(pa, la, pb, lb, torch.empty(a, b, device='cuda'))
    difference = float((ours - theirs).abs().max())
    samples = measure({'pair_kl': lambda: E.discover_pair_kl(pa, la, pb, lb, out=ours), 'torch_pair_kl': lambda: torch_pair_kl(pa, la, pb, lb, theirs)}, reps)
    ms = _ms(samples)
    floors = dict(valu_ms=3 * a * b * n / VALU_PEAK * 1e3, hbm_ms=4 * (2 * (a + b) * n + a * b) / HBM_PEAK * 1e3)
    med = ms['pair_kl']['median']
    row = dict(shape=name, leg='pair_kl', A=a, B=b, N=n, triples=a * b * n, floors_ms={k: round(v, 4) for k, v in floors.items()}, ms=ms,
               fraction_of_floor={k: round(v / med, 4) for k, v in floors.items()}, speedup=round(ms['torch_pair_kl']['median'] / med, 2),
               bar_met=bool(med <= ms['torch_pair_kl']['median']), max_abs_difference=difference, largest_D=float(theirs.max()))
    print(json.dumps(row), flush=True)
    return row


def bench_discover(reps, grid=(64, 64), segments=6, size=(1024, 1024)):
    h, w = grid
    cells = h * w
    gen = torch.Generator(device='cuda').manual_seed(7)
    seg = (torch.arange(cells, device='cuda') * segments) // cells
    own = (seg[:, None] == seg[None, :]).float()
    sums = (0.9 * own / own.sum(dim=1, keepdim=True) + 0.1 / cells) * (1 + 0.01 * (2 * torch.rand(cells, cells, generator=gen, device='cuda') - 1))
    aff = SelfAffinity(sums.contiguous(), grid, 1, 1)
    kw = dict(anchors=16, threshold=1.1, iterations=3, size=size)
    ours, theirs = aff.discover(**kw), torch_discover(aff, **kw)
    agree = float((ours.labels == theirs[0]).float().mean())
    ms = _ms(measure({'discover': lambda: aff.discover(**kw), 'torch_discover': lambda: torch_discover(aff, **kw)}, reps))
    row = dict(shape='discover_64x64_to_1024', leg='discover', grid=list(grid), size=list(size), proposals=ours.n, planted_segments=segments, ms=ms,
               speedup=round(ms['torch_discover']['median'] / ms['discover']['median'], 2),
               bar_met=bool(ms['discover']['median'] <= ms['torch_discover']['median']), label_agreement=agree)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'discover.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rows = [bench_pair_kl(name, *shape, args.reps) for name, shape in SHAPES.items()] + [bench_discover(args.reps)]
    failed = [r['shape'] for r in rows if not r['bar_met']]
    bar = dict(ratio=1.0, met=not failed, failed=failed)
    res = dict(workload=f'pair_kl at {SHAPES} as (A, B, N), f32, and SelfAffinity.discover(anchors=16, iterations=3) on a planted 64 x 64 affinity '
                        f'labelled at 1024 x 1024; one sample = one call of a leg between two HIP events, legs alternating, {args.reps} samples '
                        f'per leg after 3 warm-up rounds',
               yardstick='torch on the same GPU: broadcast differences, a product and a sum over cells, chunked over A so that [chunk, B, N] f32 '
                         'takes at most 1 GiB; for discover the same loop with torch in place of the four passes',
               peaks=dict(hbm_bytes_per_s=HBM_PEAK, valu_f32_lane_ops_per_s=VALU_PEAK), device=torch.cuda.get_device_name(0),
               kernel_shas=build.kernel_shas(build.DISCOVER_LIB), bar=bar, results=rows)
    print(json.dumps(dict(bar=bar)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
