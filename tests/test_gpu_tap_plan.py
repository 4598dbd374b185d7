"""What the tap planner decides (daam_amd/csrc/daam_tap_api.hip: tap_group -> tap_route -> tap_tables -> tap_launch_kind), pinned
through the raw C ABI with literal expected values: the kernels of a launch (``daam_last_kernels``), their number, how many ran on
side streams and the longest step chain (``daam_last_flush``), and grid / block / LDS bytes (``daam_last_launch``: the grid summed
over the launch's kernels, the LDS of the kernel launched last -- the main one).

The expected values were read off a library built from the commit BEFORE the tap host path was split into stages (this file passes
against that library through ``DAAM_HIP_LIB``), so they pin the planner's behaviour across that refactor and for whoever adds the next
kind: one launch per distinct kind in first-seen order, side kinds first and the largest last, the re-routing order mixed head dims ->
chunk, slab, pair, walk.

Common setup: fp16 Q / K and fp16 sums, 77 tokens, batch 2, three deferred steps (unless a case says otherwise)."""
import ctypes
import hashlib
import math

import numpy as np
import pytest
import torch

from test_gpu_layouts import BATCH, DEV, ROUTES, _configure, _qk_desc
from test_gpu_parity import _dev, _engine, _qk

pytestmark = pytest.mark.gpu

SD15 = [(40, 8, 16), (80, 4, 8), (160, 2, 8)]                # (head_dim, heads, side); hw 256 at head_dim 40: the slab's tail split makes a second entry
D64 = (64, 2, 16)
NO_SLAB_CHUNK = dict(DAAM_TAP_SLAB='0', DAAM_TAP_CHUNKED='0')

# case -> what to run (see _observe) and what the planner must report
CASES = {
    # 1-4: the SD-v1.5 head dims in one launch, on each of the four routes a mixed launch can take
    'sd15_slab': dict(layers=SD15, env={},
                      kernels=['tap_slab_kernel'], flush=(1, 0, 3), launch=(32, 512, 72720)),
    'sd15_chunk': dict(layers=SD15, env=dict(DAAM_TAP_SLAB='0'),
                       kernels=['tap_chunk_kernel'], flush=(1, 0, 3), launch=(24, 256, 37888)),
    'sd15_three_kernels': dict(layers=SD15, env=NO_SLAB_CHUNK,
                               kernels=['tap_d64_kernel', 'tap_wide_kernel', 'tap_wide_kernel'], flush=(3, 2, 3), launch=(32, 256, 37888)),
    'sd15_three_kernels_one_stream': dict(layers=SD15, env=dict(NO_SLAB_CHUNK, DAAM_NO_SIDE_STREAM='1'),
                                          kernels=['tap_d64_kernel', 'tap_wide_kernel', 'tap_wide_kernel'], flush=(3, 0, 3), launch=(32, 256, 97792)),
    # 5: head_dim 64 -- eight waves when every layer of the launch has head_dim 64 (and DAAM_TAP_W8 is not 0), else four
    'd64_w8': dict(layers=[D64, D64], env={}, kernels=['tap_d64_kernel'], flush=(1, 0, 3), launch=(8, 512, 54272)),
    'd64_w4': dict(layers=[D64, D64], env=dict(DAAM_TAP_W8='0'), kernels=['tap_d64_kernel'], flush=(1, 0, 3), launch=(8, 256, 37888)),
    'd64_with_d40': dict(layers=[D64, (40, 8, 8)], env=NO_SLAB_CHUNK, kernels=['tap_d64_kernel'], flush=(1, 0, 3), launch=(16, 256, 37888)),
    # 6: tap_mfma_kernel layers with different k-step counts stay separate launches
    'mfma_per_kstep_count': dict(layers=[D64, (80, 4, 8)], env=dict(DAAM_NO_D64='1'),
                                 kernels=['tap_mfma_kernel', 'tap_mfma_kernel'], flush=(2, 1, 3), launch=(16, 256, 28672)),
    # 7: a generation chain and fixed-K chains on the same Q pointers (probes)
    'pair_two_pairs': dict(layers=[D64] * 4, env=dict(DAAM_TAP_PAIR='1'), shared_q=True,
                           kernels=['tap_pair_kernel'], flush=(1, 0, 3), launch=(8, 512, 64512)),
    'pair_and_single': dict(layers=[D64] * 3, env=dict(DAAM_TAP_PAIR='1'), shared_q=True,
                            kernels=['tap_d64_kernel', 'tap_pair_kernel'], flush=(2, 1, 3), launch=(16, 512, 64512)),
    # 8: time windows [0, 1, 2] -- three steps are three windows of the layer (a walk), one step is one window (no walk)
    'walk': dict(layers=[D64], env=dict(DAAM_TAP_WALK='1'), bins=[0, 1, 2], kernels=['tap_walk_kernel'], flush=(1, 0, 1), launch=(8, 512, 73984)),
    'walk_single_window': dict(layers=[D64], env=dict(DAAM_TAP_WALK='1'), bins=[0, 1, 2], steps=1,
                               kernels=['tap_d64_kernel'], flush=(1, 0, 1), launch=(8, 512, 54272)),
}

# 9: immediate daam_tap_qk -- route of test_gpu_layouts.ROUTES (its kernel name and block size), torch dtype, (grid, LDS bytes)
IMMEDIATE = {
    'd64_immediate': (torch.float16, (8, 37888)),
    'wide80': (torch.float16, (8, 60928)),
    'wide160': (torch.float16, (8, 97792)),
    'any_shape_f32': (torch.float32, (8, 21760)),
}

_cache = {}


def _last(nat, eng):
    """(sorted kernel names, (kernels, side streams, longest chain), (grid, block, LDS bytes)) of the last tap launch."""
    ints = [ctypes.c_int() for _ in range(6)]
    nat.check(eng.lib.daam_last_flush(eng.ctx, *(ctypes.byref(v) for v in ints[:3]), None))
    nat.check(eng.lib.daam_last_launch(eng.ctx, 0, *(ctypes.byref(v) for v in ints[3:])))
    vals = [v.value for v in ints]
    return sorted(eng.last_kernels(0).split('+')), tuple(vals[:3]), tuple(vals[3:])


def _raw_engine(dtype, layers, bins=None):
    eng = _engine(n_layers=len(layers), accumulate='exact', defer_steps=0, time_bins=bins)
    eng._require_device(torch.empty(1, device=DEV))
    eng._ensure_ctx(dtype)
    for i, (_, heads, side) in enumerate(layers):
        eng._ensure_layer(i, BATCH * heads - (BATCH * heads) // 2, side, 1)
        eng._touch(i)
    return eng


def _observe(monkeypatch, case):
    """One deferred launch of ``CASES[case]``: a chain of ``steps`` steps per layer.  ``shared_q``: every layer reads layer 0's Q
    tensors, and every layer but the first has ONE K tensor for all of its steps (a probe).  Returns what the planner reported and
    a digest of every layer's sums."""
    if case in _cache:
        return _cache[case]
    from daam_amd import _native as nat
    spec = CASES[case]
    layers, steps, shared = spec['layers'], spec.get('steps', 3), spec.get('shared_q', False)
    _configure(monkeypatch, spec['env'])
    for var in ('DAAM_NO_SIDE_STREAM', 'DAAM_NO_START_GATE'):
        if var not in spec['env']:
            monkeypatch.delenv(var, raising=False)
    eng = _raw_engine(torch.float16, layers, spec.get('bins'))
    rng = np.random.default_rng(11)
    keep = []                                                 # the launch reads the tensors: keep them alive until it ran
    for i, (d, heads, side) in enumerate(layers):
        data = [_qk(rng, BATCH, heads, side * side, d, np.float16, sos_gain=1.0 + 0.5 * s) for s in range(steps)]
        keep.append([(_dev(q), _dev(k)) for q, k in data])
    for s in range(steps):
        for i, (d, heads, side) in enumerate(layers):
            q = keep[0][s][0] if shared else keep[i][s][0]
            k = keep[i][0][1] if shared and i else keep[i][s][1]
            desc = nat.QKDesc(in_dtype=0, batch=BATCH, heads=heads, hw=side * side, tokens=77, head_dim=d, round_logits=1, scale=float(d ** -0.5),
                              q_stride_b=q.stride(0), q_stride_h=d, q_stride_p=q.stride(1),
                              k_stride_b=k.stride(0), k_stride_h=d, k_stride_t=k.stride(1))
            nat.check(eng.lib.daam_tap_qk_enqueue(eng.ctx, i, q.data_ptr(), k.data_ptr(), ctypes.byref(desc)))
    nat.check(eng.lib.daam_tap_flush(eng.ctx, eng.stream))
    torch.cuda.synchronize()
    kernels, flush, launch = _last(nat, eng)
    sums = [eng.acc[i].clone().cpu() for i in range(len(layers))]
    eng.close()
    for t in sums:
        assert not torch.isnan(t.float()).any() and float(t.float().abs().max()) > 0
    digest = [hashlib.sha256(t.view(torch.int16).numpy().tobytes()).hexdigest() for t in sums]
    _cache[case] = dict(kernels=kernels, flush=flush, launch=launch, digest=digest)
    return _cache[case]


@pytest.mark.parametrize('case', list(CASES))
def test_deferred_launch_plan(case, monkeypatch):
    got = _observe(monkeypatch, case)
    print(f'{case}: kernels {got["kernels"]} flush {got["flush"]} launch {got["launch"]}')
    want = CASES[case]
    assert got['kernels'] == want['kernels']
    assert got['flush'] == want['flush']
    assert got['launch'] == want['launch']


def test_every_route_of_the_mixed_launch_leaves_the_same_bits(monkeypatch):
    """Slab, chunk, three kernels on side streams, three kernels on one stream: bit-identical sums, as the planner's comments say."""
    base = _observe(monkeypatch, 'sd15_slab')
    for case in ('sd15_chunk', 'sd15_three_kernels', 'sd15_three_kernels_one_stream'):
        assert _observe(monkeypatch, case)['digest'] == base['digest'], case


@pytest.mark.parametrize('route', list(IMMEDIATE))
def test_immediate_tap_goes_through_the_shared_launcher(route, monkeypatch):
    from daam_amd import _native as nat
    dtype, (grid, lds) = IMMEDIATE[route]
    r = ROUTES[route]
    d, heads, side = r['d'], r['heads'], 16
    _configure(monkeypatch, r['env'])
    eng = _raw_engine(dtype, [(d, heads, side)])
    np_dt = np.float16 if dtype == torch.float16 else np.float32
    q, k = (_dev(x) for x in _qk(np.random.default_rng(5), BATCH, heads, side * side, d, np_dt, sos_gain=1.0))

    class _T:                                                 # what _qk_desc reads of a placed tensor
        def __init__(self, t):
            self.strides = (t.stride(0), d, t.stride(1))
    desc = _qk_desc(nat, dtype, heads, side * side, d, _T(q), _T(k))
    nat.check(eng.lib.daam_tap_qk(eng.ctx, 0, q.data_ptr(), k.data_ptr(), ctypes.byref(desc), eng.stream))
    torch.cuda.synchronize()
    kernels, _, launch = _last(nat, eng)
    sums = eng.acc[0].float().cpu()
    eng.close()
    print(f'{route}: kernels {kernels} launch {launch}')
    assert (kernels, launch[1]) == ([r['kernel'][0]], r['kernel'][1])
    assert (launch[0], launch[2]) == (grid, lds)
    # one step: the probabilities of every (head, pixel) sum to one over the tokens
    half_ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -24
    np.testing.assert_allclose(sums.numpy().astype(np.float64).sum(-3), 1.0, atol=77 * half_ulp * (1 if dtype == torch.float16 else 8))
    assert math.isfinite(float(sums.sum()))
