"""The rotary pass (include/daam_rope.h) and the tapped FLUX attention call at the shape they are built for -- FLUX.1 at
1024 x 1024: bf16, 24 heads, d = 128, T = 512 text rows, P = 4096 image cells, batch 1 -- the HIP path against a plain torch
restatement on the same GPU, in one process with the legs alternating.

  (a) ``rope``          : ``engine.rope_apply`` of a double-stream call's three jobs (Q, image K, text K) into one buffer -- one launch;
  (b) ``torch_rope``    : the same rows through torch eager: diffusers' ``apply_rotary_emb`` per tensor and a ``cat``;
  (c) ``double`` / ``single``             : rotary launch + ``JointTapState.tap`` of one double-stream / one single-stream call;
  (d) ``torch_double`` / ``torch_single`` : the torch restatement of (c): the rotation, ``bmm`` over the concatenated keys, ``softmax``
                          (f32), the text columns, a sum over heads, ``add_`` -- written plainly and not tuned.

Every sample is one call of a leg between two HIP events (so it holds the host's enqueue gaps); the table reports the median and the
spread of each leg, the bytes of (a) -- every x read and every out written once, the cos / sin rows once (their re-reads per head
come out of L2) -- and the fraction of the 8 TB/s HBM peak those bytes over (a)'s median are.  The bars: (a) <= (b), each (c) <= its
(d).  The yardstick is the torch route in the same run, never an earlier number of this code.

    python tools/flux_tap_bench.py [--out profiles/flux_tap.json] [--reps 20]
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

from daam_amd import build, engine as E  # noqa: E402

HBM_PEAK = 8.0e12                            # bytes per second
HEADS, D, T, GRID = 24, 128, 512, (64, 64)
AXES, THETA = (16, 56, 56), 10000.0


def flux_table(text_rows, h, w):
    """f32 ``(cos, sin)`` [text_rows + h w, d] as FLUX builds them (float64 angles, cast, every value twice)."""
    ids = torch.zeros(text_rows + h * w, 3, dtype=torch.float64)
    ids[text_rows:, 1] = torch.arange(h, dtype=torch.float64).repeat_interleave(w)
    ids[text_rows:, 2] = torch.arange(w, dtype=torch.float64).repeat(h)
    cos, sin = [], []
    for axis, dim in enumerate(AXES):
        omega = 1.0 / THETA ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim)
        angles = torch.outer(ids[:, axis], omega)
        cos.append(angles.cos().repeat_interleave(2, dim=1).float())
        sin.append(angles.sin().repeat_interleave(2, dim=1).float())
    return torch.cat(cos, dim=1).cuda(), torch.cat(sin, dim=1).cuda()


def apply_rotary_emb(x, cos, sin):
    """diffusers' ``apply_rotary_emb(x, (cos, sin), use_real=True, use_real_unbind_dim=-1)`` on x [b, heads, rows, d]."""
    c, s = cos[None, None], sin[None, None]
    real, imag = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    turned = torch.stack([-imag, real], dim=-1).flatten(3)
    return (x.float() * c + turned.float() * s).to(x.dtype)


def split(t):
    return t.view(t.shape[0], t.shape[1], HEADS, D).transpose(1, 2)


def torch_tap(q, keys, tokens, scale, sums):
    """q [1, heads, P, d], keys [1, heads, T + P, d] (text rows first), both rotated."""
    probs = torch.softmax(torch.bmm(q[0], keys[0].transpose(1, 2)) * scale, dim=-1, dtype=torch.float32)
    sums.add_(probs[:, :, :tokens].sum(dim=0).t())
    return sums


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flux_tap.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    h, w = GRID
    P, C, scale = h * w, HEADS * D, D ** -0.5
    gen = torch.Generator(device='cuda').manual_seed(5)
    q, k_img = ((0.7 * torch.randn(1, P, C, generator=gen, device='cuda')).bfloat16() for _ in range(2))
    k_txt = (0.7 * torch.randn(1, T, C, generator=gen, device='cuda')).bfloat16()
    k_all = (0.7 * torch.randn(1, T + P, C, generator=gen, device='cuda')).bfloat16()          # a single-stream call's keys
    cos, sin = flux_table(T, h, w)
    buf = torch.empty(1, T + 2 * P, C, dtype=torch.bfloat16, device='cuda')
    rq, rki, rkt, rk = buf[:, T + P:], buf[:, T:T + P], buf[:, :T], buf[:, :T + P]
    image, text = (cos[T:], sin[T:], HEADS), (cos[:T], sin[:T], HEADS)
    double_jobs = [(q, rq, *image), (k_img, rki, *image), (k_txt, rkt, *text)]
    single_jobs = [(q, rq, *image), (k_all, rk, cos, sin, HEADS)]
    state = E.JointTapState(h, w, T)

    def rope():
        E.rope_apply(double_jobs, D)

    def torch_rope():
        keys = torch.cat([apply_rotary_emb(split(k_txt), *text[:2]), apply_rotary_emb(split(k_img), *image[:2])], dim=2)
        return apply_rotary_emb(split(q), *image[:2]), keys

    def double():
        E.rope_apply(double_jobs, D)
        state.tap(rq, rkt, rki, HEADS, scale)

    def single():
        E.rope_apply(single_jobs, D)
        state.tap(rq, rkt, rki, HEADS, scale)

    theirs = torch.zeros(T, P, device='cuda')

    def torch_double():
        return torch_tap(*torch_rope(), T, scale, theirs)

    def torch_single():
        return torch_tap(apply_rotary_emb(split(q), *image[:2]), apply_rotary_emb(split(k_all), cos, sin), T, scale, theirs)

    # the two routes agree: the rotation in every bit, the sums of one call closely
    rope()
    tq, tkeys = torch_rope()
    rotation_equal = bool(torch.equal(split(rq), tq) and torch.equal(split(buf[:, :T + P]), tkeys))
    double()
    ours = state.sums.clone()
    difference = float((ours - torch_double()).abs().max())
    fns = dict(rope=rope, torch_rope=torch_rope, double=double, torch_double=torch_double, single=single, torch_single=torch_single)
    samples = measure(fns, args.reps)
    ms = {leg: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for leg, v in samples.items()}
    rope_bytes = 2 * 2 * (2 * P + T) * C + 2 * 4 * (T + P) * D                    # x read, out written; cos and sin rows once
    seconds = ms['rope']['median'] * 1e-3
    bars = {ours_: dict(yardstick=theirs_, met=bool(ms[ours_]['median'] <= ms[theirs_]['median']),
                        speedup=round(ms[theirs_]['median'] / ms[ours_]['median'], 2))
            for ours_, theirs_ in (('rope', 'torch_rope'), ('double', 'torch_double'), ('single', 'torch_single'))}
    res = dict(workload=f'one FLUX.1 attention call at 1024 x 1024: bf16, batch 1, {HEADS} heads, d = {D}, T = {T}, P = {P}; one sample = one call of a '
                        f'leg between two HIP events, legs alternating, {args.reps} samples per leg after 3 warm-up rounds',
               yardstick='torch on the same GPU in the same run: apply_rotary_emb + cat; then bmm over the concatenated keys, softmax in f32, the '
                         'text columns, a sum over heads, add_',
               device=torch.cuda.get_device_name(0), kernel_shas=dict(rope=build.kernel_shas(build.ROPE_LIB), joint=build.kernel_shas(build.JOINT_LIB)),
               ms=ms, rope_bytes=rope_bytes, rope_bytes_per_s=round(rope_bytes / seconds, 1), hbm_peak_bytes_per_s=HBM_PEAK,
               rope_fraction_of_hbm_peak=round(rope_bytes / seconds / HBM_PEAK, 4), rotation_bit_equal_to_torch=rotation_equal,
               double_max_abs_difference=difference, bars=bars, all_bars_met=all(b['met'] for b in bars.values()))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
