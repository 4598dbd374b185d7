"""Probes at the headline's size: SDXL-base-1.0 topology 1024 x 1024, fp16, 50 denoising steps with one distinct Q / K set per step
(as bench.py), traced with P = 0, 1, 2 and 4 probes; and the SD-v1.5 topology (head_dim 40 / 80 / 160, the slab kernel) with P = 1.
Reports, from the library's HIP-event history (daam_profile_enable(ctx, 2)):

  * the tap launch (one launch per generation: the generation's chains and every probe's chains over the same recorded Q), with the
    head_dim-64 chains paired on tap_pair_kernel (DAAM_TAP_PAIR=1) and without (the default: every chain alone on tap_d64_kernel);
  * the grouped probe finalize (compute_probe_heat_maps: one daam_finalize_groups call, groups = probes).

Byte models: ``tap_bytes`` = what the launch moves -- Q + K of the conditional half (50 steps) once per kernel chain that reads them
(SDXL paired: ceil((1 + P) / 2) reads of Q; unpaired, and SD-v1.5's slab chains: 1 + P) + (1 + P) sum sets written once;
``tap_min_bytes`` = Q + K read once + (1 + P) sum sets.  Fraction of the 8 TB/s HBM peak = tap_bytes /
time / 8e12.  The probe finalize reads every probe's sum planes once and writes P [77, 64, 64] f32 maps.

    python tools/probe_bench.py [--out profiles/probes.json] [--reps 3]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from daam_amd import _native as nat  # noqa: E402
from daam_amd.engine import HeatMapEngine  # noqa: E402

PEAK = 8e12


def history(eng, which, n):
    buf = (ctypes.c_float * n)()
    got = ctypes.c_int()
    nat.check(eng.lib.daam_profile_history(eng.ctx, which, buf, n, ctypes.byref(got)))
    return [buf[i] for i in range(got.value)]


def run(kind, latent, n_probes, steps, reps, calls, qk_step, acc, pair=True):
    n_layers = max(a[0] for step in calls for a in step) + 1
    if pair:                                                    # read when the engine creates its context
        os.environ['DAAM_TAP_PAIR'] = '1'
    else:
        os.environ.pop('DAAM_TAP_PAIR', None)
    eng = HeatMapEngine(n_layers, tokens=77, out_side=64, defer_steps=64, n_probes=n_probes)
    g = torch.Generator(device='cuda').manual_seed(5)
    for a in calls[0]:                                          # one probe key set per layer, fixed over all steps
        layer, key = a[0], a[2]
        if n_probes:
            eng.set_probe_keys(layer, torch.randn(n_probes, 77, key.shape[-1], generator=g, device='cuda', dtype=key.dtype))
    tap_ms, fin_ms = [], []
    for r in range(reps + 1):
        eng.clear()
        for t in range(steps):
            for a in calls[t % len(calls)]:
                eng.tap_qk(*a)
        if r == 0:
            eng.flush()                                         # context + layers exist; warm-up generation
            nat.check(eng.lib.daam_profile_enable(eng.ctx, 2))
            continue
        eng.flush()
        tap_ms.append(history(eng, 0, 1)[-1])
        if n_probes:
            eng.probe_heat_maps(list(range(n_probes)), 1, [77] * n_probes)
            fin_ms.append(history(eng, 1, 1)[-1])
    torch.cuda.synchronize()
    kernels = eng.last_kernels(0)
    flush = eng.last_flush()
    fin_kernels = eng.last_kernels(1) if n_probes else ''
    eng.close()
    t = statistics.median(tap_ms)
    q_reads = -(-(1 + n_probes) // 2) if (pair and kind == 'sdxl') else 1 + n_probes
    tap_b = q_reads * steps * qk_step + (1 + n_probes) * acc
    min_b = steps * qk_step + (1 + n_probes) * acc
    row = dict(topology=kind, n_probes=n_probes, pairing=pair, tap_kernels=kernels, tap_kernel_launches=flush['kernels'], max_steps=flush['max_steps'],
               tap_launch_ms=round(t, 4), tap_bytes=tap_b, tap_frac_peak=round(tap_b / (t * 1e-3) / PEAK, 3), tap_min_bytes=min_b,
               samples=dict(tap=tap_ms))
    if n_probes:
        f = statistics.median(fin_ms)
        fin_b = n_probes * (acc + 77 * 64 * 64 * 4)
        row.update(probe_finalize_kernels=fin_kernels, probe_finalize_ms=round(f, 4), probe_finalize_bytes=fin_b,
                   probe_finalize_frac_peak=round(fin_b / (f * 1e-3) / PEAK, 3))
        row['samples']['finalize'] = fin_ms
    print(json.dumps({k: v for k, v in row.items() if k != 'samples'}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'probes.json'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    args = ap.parse_args()
    rows = []
    for kind, latent, side, counts in (('sdxl', 128, 64, (0, 1, 2, 4)), ('sd15', 64, 64, (0, 1))):
        layers = bench.topology(kind, latent)
        sets = bench.make_inputs(layers, args.steps, 'cuda', seed=11)
        calls = bench.call_lists(layers, sets, side)
        _, qk_step, acc = bench.tap_bytes(layers, 1, 2, True)
        for n_probes in counts:
            for pair in ((True, False) if n_probes and kind == 'sdxl' else (True,)):
                rows.append(run(kind, latent, n_probes, args.steps, args.reps, calls, qk_step, acc, pair))
        del sets, calls
        torch.cuda.empty_cache()
    res = dict(workload='SDXL-base-1.0 topology 1024x1024 and SD-v1.5 512x512, fp16 Q/K and sums, %d steps, one distinct Q/K set per '
                        'step; pairing = chains that share Q paired on tap_pair_kernel' % args.steps,
               device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
