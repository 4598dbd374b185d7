"""Token co-attention at the SDXL-1024 and SD-v1.5 topologies: one ``HeatMapEngine.token_gram`` call (``daam_token_gram``: the running
sums read once, ending on the matrix cores) against the route there was before it, in one process on the same buffers:

  * ``token_gram`` : one call for every key x 77 rows (fp16 sums: the 16-bit path);
  * ``torch``      : layer by layer ``torch.bmm`` of the f32 copy of the layer's views with its transpose;
  * ``wide``       : the library's f32 path on the same fp16 planes, reached through the raw ABI with ``n_win = 2`` and
                     ``win_stride = 0`` (every plane added to itself: the Gram of 2 A, the second read served by the caches) -- an
                     upper bound of what the f32 path costs on these bytes, which is what the dispatch between the paths rests on.

Synthetic fp16 sums in [0, 64).  Every sample is one call of a leg between two HIP events after warm-up rounds, the legs
alternating; the table reports median, min and max.  ``peak_fraction`` = plane bytes over the ``token_gram`` median over 8 TB/s.
``agree``: both routes within 1e-3 of each other relative to the largest entry (a plausibility check; the bound is held by
tests/test_gpu_token_gram.py).  One topology per process; a second run adds its row to the same file:

    timeout -k 10 300 python tools/token_gram_bench.py --topology sdxl && timeout -k 10 300 python tools/token_gram_bench.py --topology sd15
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
TOPOLOGIES = {                                                   # (side, heads, factor) per layer
    'sdxl': [(64, 10, 1)] * 10 + [(32, 20, 2)] * 50,
    'sd15': [(64, 8, 1)] * 5 + [(32, 8, 2)] * 5 + [(16, 8, 4)] * 5 + [(8, 8, 8)],
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
        acc.copy_((torch.rand(acc.shape, generator=g, device='cuda:0', dtype=torch.float32) * 64.0).to(acc.dtype))
        plane_bytes += acc.numel() * acc.element_size()
    return eng, plane_bytes


def torch_route(eng):
    out = []
    for layer in sorted(eng.touched):
        a = eng.acc[layer].reshape(eng.acc[layer].shape[0], ROWS, -1).float()
        out.append(torch.bmm(a, a.transpose(1, 2)))
    return torch.cat(out)


def wide_route(eng, keys):
    """The same keys with n_win = 2, win_stride = 0 through the raw ABI: the f32 path on the fp16 planes."""
    lib = nat.load_analysis()
    views = dict(eng.items())
    arr = (nat.KeyPlanes * len(keys))(*[nat.KeyPlanes(base=views[k].data_ptr(), win_stride=0, h=views[k].shape[-2], w=views[k].shape[-1],
                                                      n_win=2, pad=0) for k in keys])
    desc = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to('cuda:0')
    need = lib.daam_token_gram_scratch_bytes(len(keys), ROWS, 64 * 64)
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    gram = torch.empty(len(keys), ROWS, ROWS, dtype=torch.float32, device='cuda:0')

    def call():
        nat.check_analysis(lib.daam_token_gram(desc.data_ptr(), len(keys), nat.DAAM_F16, ROWS, gram.data_ptr(), scratch.data_ptr(), need,
                                               torch.cuda.current_stream().cuda_stream))
        return gram
    return call, (desc, scratch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'token_gram.json'))
    ap.add_argument('--topology', choices=sorted(TOPOLOGIES), default='sdxl')
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng, plane_bytes = make_engine(TOPOLOGIES[args.topology])
    keys, got = eng.token_gram()
    want = torch_route(eng)
    agree = bool(((got - want).abs().max() <= 1e-3 * want.abs().max()).item())
    wide, keep = wide_route(eng, keys)
    agree_wide = bool(((wide() - 4.0 * want).abs().max() <= 4e-3 * want.abs().max()).item())
    samples = measure({'token_gram': lambda: eng.token_gram(), 'torch': lambda: torch_route(eng), 'wide': wide}, args.reps)
    med = {k: statistics.median(v) for k, v in samples.items()}
    row = dict(topology=args.topology, keys=len(keys), rows=ROWS, agree=agree, agree_wide=agree_wide, plane_bytes=plane_bytes,
               gram_bytes=got.numel() * 4,
               ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4), samples=len(v)) for k, v in samples.items()},
               peak_fraction=round(plane_bytes / (med['token_gram'] * 1e-3) / PEAK_BYTES_PER_S, 4),
               achieved_tb_per_s=round(plane_bytes / (med['token_gram'] * 1e-3) / 1e12, 3),
               over_torch=round(med['token_gram'] / med['torch'], 3), not_slower_than_torch=bool(med['token_gram'] <= 1.03 * med['torch']),
               wide_over_narrow=round(med['wide'] / med['token_gram'], 3))
    print(json.dumps(row), flush=True)
    res = dict(workload='synthetic fp16 sums in [0, 64), 77 rows; sdxl: 10 x 10 x 64^2 + 50 x 20 x 32^2 planes per row (1100 keys); sd15: 5 x 8 '
                        'x 64^2 + 5 x 8 x 32^2 + 5 x 8 x 16^2 + 8 x 8^2 (128 keys); one sample = one call of a leg between two HIP events; '
                        f'{args.reps} samples after warm-up',
               results={})
    if os.path.exists(args.out):
        with open(args.out) as f:
            res['results'] = json.load(f).get('results', {})
    res['device'] = torch.cuda.get_device_name(0)
    res['kernel_shas'] = {k: v for k, v in build.kernel_shas(build.ANALYSIS_OUT).items() if 'token_gram' in k}
    res['results'][args.topology] = row
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
