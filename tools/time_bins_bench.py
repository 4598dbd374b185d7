"""Time windows at the headline's size: SDXL-base-1.0 topology 1024 x 1024, fp16, 50 denoising steps with one distinct Q / K
set per step (as bench.py), traced with 1, 10 and 50 time windows.  Reports, from the library's HIP-event history
(daam_profile_enable(ctx, 2)):

  * the tap launch (one launch per generation, every window's sums written once: fresh windows are not read);
  * the per-window finalize (compute_time_heat_maps: one daam_finalize_bins call per 64 windows, every window's planes);
  * the whole-generation range finalize (windows [0, n) added per key by the reduction kernel, then the f32 finalize classes).

Algorithmic bytes: Q + K of the conditional half read once (50 steps), each window's sums written once; the per-window finalize
reads every window's planes once; the range finalize reads every window's planes, writes and re-reads the f32 scratch planes.
The fraction of the 8 TB/s HBM peak is bytes / time / 8e12.

``--walk`` adds a leg with ``DAAM_TAP_WALK=1`` (tap_walk_kernel: one workgroup walks a layer's windows) for 10 and 50
windows.  Its generations alternate with the unswitched engine's, repetition by repetition, in the same process: the yardstick for
the walk kernel is the unswitched launch of the same run, not a figure from another box.  Its rows carry ``tap_walk: true``.

    python tools/time_bins_bench.py [--out profiles/time_bins.json] [--reps 3] [--walk]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'time_bins.json'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--walk', action='store_true', help='also measure 10 and 50 windows with DAAM_TAP_WALK=1')
    args = ap.parse_args()
    steps = args.steps
    layers = bench.topology('sdxl', 128)
    sets = bench.make_inputs(layers, steps, 'cuda', seed=11)
    calls = bench.call_lists(layers, sets, 64)
    n_layers = max(l[0] for l in layers) + 1
    _, qk_step, acc = bench.tap_bytes(layers, 1, 2, True)
    plane_out = 77 * 64 * 64 * 4
    acc32 = acc * 2
    rows = []
    def make_engine(bins, walk):
        # the library reads the switch when the engine creates its context (at the first tap)
        if walk:
            os.environ['DAAM_TAP_WALK'] = '1'
        else:
            os.environ.pop('DAAM_TAP_WALK', None)
        eng = HeatMapEngine(n_layers, tokens=77, out_side=64, defer_steps=64, time_bins=bins)
        for a in calls[0]:
            eng.tap_qk(*a)
        os.environ.pop('DAAM_TAP_WALK', None)
        return eng

    for n_bins in (1, 10, 50):
        bins = [round(i * steps / n_bins) for i in range(n_bins)]
        legs = [False, True] if args.walk and n_bins > 1 else [False]
        engines = {walk: make_engine(bins, walk) for walk in legs}
        times = {walk: ([], [], []) for walk in legs}
        for r in range(args.reps + 1):
            for walk in legs:                                   # alternating: one generation each per repetition
                eng = engines[walk]
                tap_ms, per_ms, rng_ms = times[walk]
                eng.clear()
                for t in range(steps):
                    for a in calls[t]:
                        eng.tap_qk(*a)
                if r == 0:
                    eng.flush()                                 # context + layers exist; warm-up generation
                    nat.check(eng.lib.daam_profile_enable(eng.ctx, 2))
                    continue
                eng.flush()
                tap_ms.append(history(eng, 0, 1)[-1])
                groups = [(w, w + 1, 0) for w in range(n_bins)]
                eng.time_heat_maps(groups, 1, [77])
                n_calls = -(-n_bins // 64)
                per_ms.append(sum(history(eng, 1, n_calls)[-n_calls:]))
                eng.time_heat_maps([(0, n_bins, 0)], 1, [77])
                rng_ms.append(history(eng, 1, 1)[-1])
        torch.cuda.synchronize()
        for walk in legs:
            eng = engines[walk]
            tap_ms, per_ms, rng_ms = times[walk]
            launches = eng.last_flush()['launches']
            kernels = eng.last_kernels(0)
            fin_kernels = eng.last_kernels(1)
            eng.close()
            tap_b = steps * qk_step + n_bins * acc
            per_b = n_bins * (acc + plane_out)
            rng_b = n_bins * acc + 2 * acc32 + plane_out if n_bins > 1 else acc + plane_out
            t, p, g = statistics.median(tap_ms), statistics.median(per_ms), statistics.median(rng_ms)
            rows.append(dict(n_bins=n_bins, tap_walk=walk, time_bins=bins, tap_kernels=kernels, range_finalize_kernels=fin_kernels,
                             tap_launch_ms=round(t, 4), tap_bytes=tap_b, tap_frac_peak=round(tap_b / (t * 1e-3) / PEAK, 3),
                             per_window_finalize_ms=round(p, 4), per_window_bytes=per_b,
                             per_window_frac_peak=round(per_b / (p * 1e-3) / PEAK, 3),
                             range_finalize_ms=round(g, 4), range_bytes=rng_b, range_frac_peak=round(rng_b / (g * 1e-3) / PEAK, 3),
                             samples=dict(tap=tap_ms, per_window=per_ms, range=rng_ms), tap_launches_total=launches))
            print(json.dumps({k: v for k, v in rows[-1].items() if k not in ('samples', 'time_bins')}), flush=True)
    res = dict(workload='SDXL-base-1.0 topology 1024x1024, fp16 Q/K and sums, 50 steps, one distinct Q/K set per step',
               device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, qk_bytes_per_step=qk_step, sum_bytes_per_window=acc,
               results=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
