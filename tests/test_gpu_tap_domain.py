"""Every tap route's running sums against the float64 softmax PER PROBABILITY (``tests/_tap_domain.py`` builds the reference and
derives the bound from the number formats; ``tests/test_tap_domain_cpu.py`` holds both, and shows what they catch that
``2 half_ulp max(1, max want)`` cannot: fp16-subnormal probabilities flushed, a truncating conversion, minor tokens exchanged,
un-masked padding slots, a low-precision exponential).

  routes      every entry of tests/test_gpu_layouts.py::ROUTES and tests/test_gpu_softmax_domain.py::EXTRA_ROUTES, the any-shape kernel
              on an fp16 pipeline with rounded logits, the pair route, the fused tap of ``engine.attend`` at head dims 64 and 80
  sum dtypes  an fp16 route in ``f16_exact`` and ``f16_f32acc``, a bf16 route in ``bf16_exact`` and ``bf16_f32acc``; the strict flavour
              and the f32 pipeline where those files list them
  sizes       hw 256 (exact tiles) and 576 (a cut tile); two steps on the immediate routes, three on the deferred ones; walk windows
              are judged as one-step sums; one run of 12 steps on ``d64_deferred`` in fp16 sums (sums near 3 absorb 1e-7)

Each case asserts the kernel name and block size of its run, that no input was written to, ``|got - A_n| <= E_n`` on every element
(the worst ratio per row kind is printed) and, where the sums are f32 under a 16-bit pipeline, the rounding-bias rule.  Run with
``-m gpu`` on an MI355X."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _attend_domain as ad
import _tap_domain as td
from oracle import heatmap_oracle as ho
from test_gpu_attend import _engine as _attend_engine
from test_gpu_layouts import BATCH, DEV, MODES, ROUTES, _configure, _last_launch, _qk_desc, _tap_raw
from test_gpu_parity import _dev, _engine
from test_gpu_softmax_domain import EXTRA_ROUTES

pytestmark = pytest.mark.gpu

HWS = (256, 576)
ALL_ROUTES = dict(ROUTES, **EXTRA_ROUTES)
ALL_ROUTES['any_shape_f16'] = dict(d=64, heads=2, deferred=False, env=dict(DAAM_FORCE_GENERIC='1'), kernel=('tap_generic_kernel', 256),
                                   modes=('f16_exact',), round_logits=1)


def _modes(spec):
    """Both sum dtypes of every 16-bit pipeline a route lists; ``f16_strict`` and ``f32`` as listed."""
    out = []
    for dt in ('f16', 'bf16'):
        if any(m in (f'{dt}_exact', f'{dt}_f32acc') for m in spec['modes']):
            out += [f'{dt}_exact', f'{dt}_f32acc']
    return out + [m for m in spec['modes'] if m in ('f16_strict', 'f32')]


CASES = [(r, m) for r, spec in ALL_ROUTES.items() for m in _modes(spec)]

_inputs_cache, _ref_cache = {}, {}


def _inputs(hw, heads, d, np_dt, n_steps):
    key = (hw, heads, d, str(np_dt), n_steps)
    if key not in _inputs_cache:
        _inputs_cache[key] = ad.build(hw, heads, d, np_dt, n_steps)
    return _inputs_cache[key]


def _reference(hw, heads, d, np_dt, n_steps, acc_np, upcast=False, chain=None):
    """The oracle of a case, computed once per (hw, heads, d, dtype, steps) and sum dtype; ``chain``: a named variant of the steps."""
    key = (hw, heads, d, str(np_dt), n_steps, str(acc_np), upcast, chain)
    if key not in _ref_cache:
        steps, _ = _inputs(hw, heads, d, np_dt, n_steps)
        if chain == 'fixed_k':                                # the pair route's second chain: the K of step 0 at every step
            steps = [(q, steps[0][1]) for q, _ in steps]
        _ref_cache[key] = td.reference(steps, heads, d ** -0.5, np_dt, acc_np, upcast)
    return _ref_cache[key]


def _judge(got, ref, names, np_dt, mode, what, per_window=False):
    """The bound on every element; the bias rule where the sums are f32 and the pipeline is not."""
    got = np.asarray(got, np.float64)
    if per_window:
        assert got.shape[0] == len(ref['p64']), (what, got.shape)
    td.assert_inside_bound(got, td.windows(ref, np_dt, td.sum_dtype(np_dt, MODES[mode][2])) if per_window else ref, names, what)
    if mode.endswith('_f32acc'):
        td.assert_unbiased(got, ref, names, np_dt, what, per_window)


def _run_route(route, mode, hw, n, monkeypatch):
    spec = ALL_ROUTES[route]
    np_dt, dtype, accumulate, env = MODES[mode]
    heads, d, upcast = spec['heads'], spec['d'], not spec.get('round_logits', 1)
    steps, names = _inputs(hw, heads, d, np_dt, n)
    _configure(monkeypatch, dict(spec['env'], **env))
    res = _tap_raw([(_dev(q, np_dt), _dev(k, np_dt)) for q, k in steps], heads, d, hw, dtype, accumulate, 'L0', spec['deferred'],
                   spec.get('bins'), round_logits=spec.get('round_logits', 1))
    what = f'{route} {mode} hw {hw} {n} steps'
    assert (res['name'], res['block']) == spec['kernel'], (what, res['name'], res['block'])
    assert res['intact'], f'{what}: an input storage was written to'
    ref = _reference(hw, heads, d, np_dt, n, td.sum_dtype(np_dt, accumulate), upcast)
    _judge(res['sums'].float().numpy(), ref, names, np_dt, mode, what, per_window='bins' in spec)


@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('route,mode', CASES)
def test_tap_route_per_probability(route, mode, hw, monkeypatch):
    _run_route(route, mode, hw, 3 if ALL_ROUTES[route]['deferred'] else 2, monkeypatch)


def test_twelve_steps_of_fp16_sums(monkeypatch):
    """Sums near 3 in fp16 (ulp 2^-9) take probabilities near 1e-7: absorbed by the reference's adds too, and E_n says by how much."""
    _run_route('d64_deferred', 'f16_exact', 256, 12, monkeypatch)
    ref = _reference(256, 2, 64, np.float16, 12, np.float16)
    assert ref['want'].max() > 2.9 and (ref['p64'] < 2.0 ** -23).any()


@pytest.mark.parametrize('hw', HWS)
def test_pair_route_per_probability(hw, monkeypatch):
    """Two chains on one Q (``DAAM_TAP_PAIR=1``), built as tests/test_gpu_softmax_domain.py::test_pair_route_by_row_class builds them:
    the generation's, and one whose K is the same tensor at every step."""
    from daam_amd import _native as nat
    heads, d, n = 2, 64, 3
    steps, names = _inputs(hw, heads, d, np.float16, n)
    _configure(monkeypatch, dict(DAAM_TAP_PAIR='1'))
    eng = _engine(n_layers=2, accumulate='exact', defer_steps=0)
    eng._require_device(torch.empty(1, device=DEV))
    eng._ensure_ctx(torch.float16)
    for layer in range(2):
        eng._ensure_layer(layer, BATCH * heads - (BATCH * heads) // 2, math.isqrt(hw), 1)
        eng._touch(layer)
    dev = [(_dev(q), _dev(k)) for q, k in steps]
    before = [(q.clone(), k.clone()) for q, k in dev]

    class _T:                                                 # what _qk_desc reads of a placed tensor
        def __init__(self, t):
            self.strides = (t.stride(0), d, t.stride(1))
    desc = _qk_desc(nat, torch.float16, heads, hw, d, _T(dev[0][0]), _T(dev[0][1]))
    for q, k in dev:
        for layer, key in ((0, k), (1, dev[0][1])):
            nat.check(eng.lib.daam_tap_qk_enqueue(eng.ctx, layer, q.data_ptr(), key.data_ptr(), ctypes.byref(desc)))
    nat.check(eng.lib.daam_tap_flush(eng.ctx, eng.stream))
    torch.cuda.synchronize()
    name, block = _last_launch(nat, eng)
    got = [eng.acc[layer].float().cpu().numpy() for layer in range(2)]
    eng.close()
    assert (name, block) == ('tap_pair_kernel', 512), (name, block)
    assert all(torch.equal(a, c) and torch.equal(b, e) for (a, b), (c, e) in zip(dev, before)), 'an input was written to'
    for layer, chain in enumerate((None, 'fixed_k')):
        ref = _reference(hw, heads, d, np.float16, n, np.float16, chain=chain)
        _judge(got[layer], ref, names, np.float16, 'f16_exact', f'pair chain {"AB"[layer]} hw {hw}')


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)      # exact: the values are the dtype's


@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('d,heads', [(64, 2), (80, 4)])
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_fused_tap_per_probability(dt, d, heads, hw, accumulate, monkeypatch):
    """The sums ``engine.attend`` leaves with ``tapped=True``, two calls."""
    mode = f'{dt}_{"exact" if accumulate == "exact" else "f32acc"}'
    np_dt, dtype, _, _ = MODES[mode]
    n, what = 2, f'fused tap {mode} d {d} hw {hw}'
    steps, names = _inputs(hw, heads, d, np_dt, n)
    _configure(monkeypatch, {})
    eng = _attend_engine(accumulate=accumulate)
    for (q, k), v in zip(steps, ad.values('plain', heads, d, np_dt, n)):
        tq, tk, tv = _t(q, dtype), _t(k, dtype), _t(v, dtype)
        before = [x.clone() for x in (tq, tk, tv)]
        out = eng.attend(0, tq, tk, tv, heads, d ** -0.5, 1, True, tapped=True)
        assert out is not None and out.shape == tq.shape and out.dtype == dtype, what
        assert eng.last_kernels(0) == '', (what, eng.last_kernels(0))       # the tap ran inside daam_attend: no tap launch of its own
        assert all(torch.equal(a, b) for a, b in zip((tq, tk, tv), before)), f'{what}: an input was written to'
    got = torch.stack([t for _, t in eng.items()]).float().cpu().numpy()
    eng.close()
    assert got.shape == (BATCH * heads - (BATCH * heads) // 2, ad.TOKENS, math.isqrt(hw), math.isqrt(hw)), (what, got.shape)
    _judge(got, _reference(hw, heads, d, np_dt, n, td.sum_dtype(np_dt, accumulate)), names, np_dt, mode, what)
