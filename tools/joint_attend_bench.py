"""The fused joint attention (include/daam_joint_attend.h) at the shapes it is built for -- SD3-medium at 1024 x 1024
(batch 2, 24 heads, P = 4096, d = 64, fp16) with a context of 154 and of 333 rows, and a FLUX-class head dim (d = 128, T = 512) --
against what a traced block did without it, in one process with the legs alternating.

  * ``fused``   : ``JointAttendState.forward`` on the whole batch, then ``JointTapState.tap_from_stats`` on the kept half: the
                  attention and the tap from one key walk;
  * ``stock``   : ``cat`` of the text and image q / k / v, ``F.scaled_dot_product_attention``, then ``JointTapState.tap`` on the kept
                  half: the model's attention plus the two-launch tap;
  * ``forward`` : the forward alone, beside its MFMA floor 4 S (T + P)^2 d.

The projections that the stock route makes a second time for the tap are timed in neither leg: they are a further saving of the
fused route.  Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps); the table reports the
median and the spread.  The aim, per shape: fused <= stock; ``bar.met`` records it (a report, not a gate: the option is opt-in).
The stand-in MMDiT's end-to-end distances from an f32 run (fused and stock) are recorded beside the timings.

    python tools/joint_attend_bench.py [--out profiles/joint_attend.json] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from daam_amd import build, engine as E  # noqa: E402

MFMA_PEAK = 2.5e15                           # dense fp16 flops per second
SHAPES = {'sd3_1024_t154': (24, 64, 64, 154, 64), 'sd3_1024_t333': (24, 64, 64, 333, 64), 'd128_t512': (24, 64, 64, 512, 128)}   # heads, h, w, T, d
BATCH = 2


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


def bench_shape(name, heads, h, w, t, d, reps):
    p = h * w
    gen = torch.Generator(device='cuda').manual_seed(5)
    img = [(0.7 * torch.randn(BATCH, p, heads * d, generator=gen, device='cuda')).half() for _ in range(3)]
    txt = [(0.7 * torch.randn(BATCH, t, heads * d, generator=gen, device='cuda')).half() for _ in range(3)]
    scale, first = d ** -0.5, BATCH // 2
    attend, ours, theirs = E.JointAttendState(), E.JointTapState(h, w, t), E.JointTapState(h, w, t)

    def fused():
        out_i, out_t, stats = attend.forward(*img, *txt, heads, scale)
        ours.tap_from_stats(img[0][first:], txt[1][first:], heads, scale, stats[first * heads * E.pad128(p):])
        return out_i, out_t

    def stock():
        q, k, v = (torch.cat([a, b], dim=1).view(BATCH, p + t, heads, d).transpose(1, 2) for a, b in zip(img, txt))
        out = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(BATCH, p + t, heads * d)
        theirs.tap(img[0][first:], txt[1][first:], img[1][first:], heads, scale)
        return out[:, :p], out[:, p:]
    (fi, ft), (si, st) = fused(), stock()
    difference = dict(out=float(max((fi.float() - si.float()).abs().max(), (ft.float() - st.float()).abs().max())),
                      planes=float((ours.sums - theirs.sums).abs().max()))
    fns = {'fused': fused, 'stock': stock, 'forward': lambda: attend.forward(*img, *txt, heads, scale)}
    samples = measure(fns, reps)
    med = {leg: statistics.median(v) for leg, v in samples.items()}
    floor = 4 * BATCH * heads * (t + p) ** 2 * d / MFMA_PEAK * 1e3
    row = dict(shape=name, batch=BATCH, heads=heads, P=p, T=t, d=d, forward_mfma_floor_ms=round(floor, 4),
               ms={key: dict(median=round(med[key], 4), min=round(min(samples[key]), 4), max=round(max(samples[key]), 4)) for key in fns},
               forward_fraction_of_floor=round(floor / med['forward'], 4), fused_over_stock=round(med['fused'] / med['stock'], 3),
               bar_met=bool(med['fused'] <= med['stock']), max_abs_difference=difference)
    print(json.dumps(row), flush=True)
    return row


def standin_distances():
    """The stand-in MMDiT of the tests, two steps: max-abs and RMS distance of the model's output from an f32 run, for the stock
    processor and for ``trace_joint(attend=True)``."""
    import _mmdit_standin as M
    import daam_amd
    rows = []
    for dtype, size in ((torch.float16, {}), (torch.bfloat16, dict(height=96, width=160))):
        runs = {}
        exact = M.make_pipe(device='cuda:0', dtype=torch.float32, seed=3)
        exact('a photo', num_inference_steps=2, **size)
        pipe = M.make_pipe(device='cuda:0', dtype=dtype, seed=3)
        pipe('a photo', num_inference_steps=2, **size)
        runs['stock'] = [o.float() for o in pipe.outputs]
        with daam_amd.trace_joint(pipe, attend=True, **size):
            pipe('a photo', num_inference_steps=2, **size)
            runs['fused'] = [o.float() for o in pipe.outputs]
        ref = [o.float() for o in exact.outputs]
        rows.append(dict(dtype=str(dtype), size=size or 'default', **{
            leg: dict(max_abs=max(float((a - b).abs().max()) for a, b in zip(outs, ref)),
                      rms=float(torch.stack([((a - b) ** 2).mean() for a, b in zip(outs, ref)]).mean().sqrt())) for leg, outs in runs.items()}))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_attend.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    rows = [bench_shape(name, *shape, args.reps) for name, shape in SHAPES.items()]
    failed = [r['shape'] for r in rows if not r['bar_met']]
    bar = dict(ratio=1.0, met=not failed, failed=failed)
    res = dict(workload=f'one joint-attention call, batch {BATCH}, fp16, shapes {SHAPES} as (heads, h, w, T, d), P = h w; one sample = one '
                        f'call of a leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               legs=dict(fused='forward on the whole batch + tap_from_stats on the kept half',
                         stock='cat of q / k / v + scaled_dot_product_attention + JointTapState.tap on the kept half',
                         forward='the forward alone'),
               not_timed='the projections the stock route repeats for its tap: a further saving of the fused route',
               peaks=dict(mfma_fp16_flops_per_s=MFMA_PEAK), device=torch.cuda.get_device_name(0),
               kernel_shas=build.kernel_shas(build.JOINT_ATTEND_LIB), bar=bar, results=rows, standin_end_to_end=standin_distances())
    print(json.dumps(dict(bar=bar)), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
