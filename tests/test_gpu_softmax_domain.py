"""Every softmax flavour of the tap kernels and of ``daam_attend`` against the numpy oracle on rows whose sum of exponentials lies
inside, above and below the window [2^-100, 2^100] in which the kernels keep their shortcut (``tests/_softmax_domain.py`` builds
the inputs and names the classes; ``tests/test_softmax_domain_cpu.py`` holds the inputs to their shares).

  flavour                                   redo branch reached through
  fp16 fast, no reference point             d64_* / wide* / walk / pair / chunk40 / slab* in the f16 modes, fp16 daam_attend
  bf16                                      d64_* / walk / chunk80_bf16 in the bf16 modes, bf16 daam_attend
  fp16 fast, token 0 as reference point     mfma (classes judged with the sum of exp(x_t - x_0): t0_low rows are its ``over``)
  strict (row maximum always)               f16_strict, round_logits = 0 (d64_upcast, any_shape_upcast), any_shape_f32

Each case is one run at hw <= 576; kernel name and block size are asserted, so a case cannot test another kernel than it names.
Tolerances are those of ``tests/test_gpu_parity.py::test_tap_qk_vs_oracle`` for every class (for fp16 sums that IS the
``2^-10 * max(1, max want)`` of ``test_tap_wide_logit_spread``): the extreme rows' logits are exact in any summation order, so no
class needs more.  Errors are reported per class: the worst row of each.

The fp16 domain (include/daam_hip.h): with a power-of-two scale the fast fp16 flavour keeps the UNSCALED q.k in
fp16, so it needs ``|q.k| <= 65504``; ``test_fp16_*`` below hold the largest in-domain value on every flavour and the first
out-of-domain one on the flavours that scale before they round (``DAAM_STRICT_EXP=1``, tap_mfma_kernel, scales that are no power
of two)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _softmax_domain as sd
from oracle import heatmap_oracle as ho
from test_gpu_attend import _engine as _attend_engine
from test_gpu_layouts import BATCH, DEV, MODES, ROUTES, _bits, _configure, _last_launch, _qk_desc, _tap_raw
from test_gpu_parity import _dev, _engine

pytestmark = pytest.mark.gpu

# routes of tests/test_gpu_layouts.py plus: round_logits = 0 on the head_dim-64 kernel and on the any-shape kernel
EXTRA_ROUTES = {
    'd64_upcast': dict(d=64, heads=2, deferred=False, env={}, kernel=('tap_d64_kernel', 256), modes=('f16_exact',), round_logits=0),
    'any_shape_upcast': dict(d=64, heads=2, deferred=False, env=dict(DAAM_FORCE_GENERIC='1'), kernel=('tap_generic_kernel', 256),
                             modes=('f16_exact',), round_logits=0),
}
# modes a route must run beyond those it lists in ROUTES: bf16 with bf16 sums and with f32 sums on the d64, walk and chunk routes
EXTRA_MODES = {'d64_immediate': ('bf16_f32acc',), 'd64_deferred': ('bf16_f32acc',), 'walk': ('bf16_exact',),
               'chunk80_bf16': ('bf16_f32acc',)}
ALL_ROUTES = dict(ROUTES, **EXTRA_ROUTES)
CASES = [(r, m) for r, spec in ALL_ROUTES.items() for m in spec['modes'] + EXTRA_MODES.get(r, ())]

_inputs_cache, _oracle_cache = {}, {}


def _n_steps(spec):
    return 3 if spec['deferred'] else 2


def _inputs(hw, heads, d, np_dt, n_steps):
    key = (hw, heads, d, str(np_dt), n_steps)
    if key not in _inputs_cache:
        _inputs_cache[key] = sd.build(hw, heads, d, np_dt, n_steps)
    return _inputs_cache[key]


def _oracle(steps, heads, scale, np_dt, acc_np, upcast=False, per_step=False):
    """Running sums [kept heads, 77, side, side] of ``steps`` (``per_step``: one window per step, [steps, kept heads, ...])."""
    def run(part):
        raw = ho.RawMaps(acc_np)
        for q, k in part:
            ho.tap(raw, 0, sd.to_bh(q, heads), sd.to_bh(k, heads), scale, latent_hw=q.shape[1], pipe_dtype=np_dt, upcast_attention=upcast)
        return np.stack([v for _, v in raw]).astype(np.float64)
    want = np.stack([run([s]) for s in steps]) if per_step else run(steps)
    assert np.isfinite(want).all()
    return want


def _tolerance(mode, want, steps):
    """tests/test_gpu_parity.py::test_tap_qk_vs_oracle."""
    half_ulp = 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11          # of a probability <= 1
    if mode == 'f32':
        return 2e-6 * max(1.0, np.abs(want).max())
    if MODES[mode][2] == 'exact':
        return 2 * half_ulp * max(1.0, want.max())                          # 1 ulp of the largest running sum
    return steps * half_ulp                                                  # one flipped probability ulp per step


def _assert_by_class(got, want, classes, tol, what, need=()):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite sums'
    worst = sd.worst_by_class(got, want, classes)
    report = ', '.join(f'{n}: {e:.3e} at head {h} pixel {p} ({rows} rows)' for n, (e, (h, p), rows) in worst.items())
    print(f'{what}: tolerance {tol:.3e}; worst row per class -- {report}')
    for name in need:
        assert name in worst, f'{what}: no {name} rows'
    bad = [n for n, (e, _, _) in worst.items() if e > tol]
    assert not bad, f'{what}: {bad} beyond {tol:.3e}; worst row per class -- {report}'
    return worst


@pytest.mark.parametrize('hw', sd.HWS)
@pytest.mark.parametrize('route,mode', CASES)
def test_tap_route_by_row_class(route, mode, hw, monkeypatch):
    spec = ALL_ROUTES[route]
    np_dt, dtype, accumulate, env = MODES[mode]
    heads, d, n, upcast = spec['heads'], spec['d'], _n_steps(spec), not spec.get('round_logits', 1)
    steps, _ = _inputs(hw, heads, d, np_dt, n)
    _configure(monkeypatch, dict(spec['env'], **env))
    res = _tap_raw([(_dev(q, np_dt), _dev(k, np_dt)) for q, k in steps], heads, d, hw, dtype, accumulate, 'L0', spec['deferred'],
                   spec.get('bins'), round_logits=spec.get('round_logits', 1))
    what = f'{route} {mode} hw {hw}'
    assert (res['name'], res['block']) == spec['kernel'], (what, res['name'], res['block'])
    binned = 'bins' in spec
    acc_np = np.float32 if accumulate == 'float32' else np_dt
    okey = (hw, heads, d, str(np_dt), str(acc_np), n, binned, upcast)
    if okey not in _oracle_cache:
        _oracle_cache[okey] = _oracle(steps, heads, d ** -0.5, np_dt, acc_np, upcast, per_step=binned)
    want = _oracle_cache[okey]
    shifted = res['name'] == 'tap_mfma_kernel' and 'DAAM_STRICT_EXP' not in env     # token 0 is that flavour's reference point
    classes = sd.pixel_classes(sd.row_classes(steps, heads, d ** -0.5, np_dt, shifted=shifted, upcast=upcast))
    need = ('plain', 'over') if shifted else sd.CLASS_NAMES
    _assert_by_class(res['sums'].float().numpy(), want, classes, _tolerance(mode, want, 1 if binned else n), what, need)
    assert res['intact'], f'{what}: an input storage was written to'
    per = 1 if binned else n
    half_ulp = 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11
    np.testing.assert_allclose(res['sums'].float().numpy().astype(np.float64).sum(-3), per, atol=per * 77 * half_ulp, err_msg=what)


@pytest.mark.parametrize('hw', sd.HWS)
def test_pair_route_by_row_class(hw, monkeypatch):
    """Two chains on one Q (``DAAM_TAP_PAIR=1``): the generation's, and one whose K is the same tensor at every step (a probe)."""
    from daam_amd import _native as nat
    heads, d, n = 2, 64, 3
    steps, _ = _inputs(hw, heads, d, np.float16, n)
    _configure(monkeypatch, dict(DAAM_TAP_PAIR='1'))
    eng = _engine(n_layers=2, accumulate='exact', defer_steps=0)
    eng._require_device(torch.empty(1, device=DEV))
    eng._ensure_ctx(torch.float16)
    for layer in range(2):
        eng._ensure_layer(layer, BATCH * heads - (BATCH * heads) // 2, math.isqrt(hw), 1)
        eng._touch(layer)
    dev = [(_dev(q), _dev(k)) for q, k in steps]

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
    for layer, chain in enumerate((steps, [(q, steps[0][1]) for q, _ in steps])):
        want = _oracle(chain, heads, d ** -0.5, np.float16, np.float16)
        classes = sd.pixel_classes(sd.row_classes(chain, heads, d ** -0.5, np.float16))
        _assert_by_class(got[layer], want, classes, _tolerance('f16_exact', want, n), f'pair chain {"AB"[layer]} hw {hw}', sd.CLASS_NAMES)
        np.testing.assert_allclose(got[layer].astype(np.float64).sum(-3), n, atol=n * 77 * 2.0 ** -11)


# ---- daam_attend with the fused tap ------------------------------------------------------------------------------------------
# the kernel of the immediate stand-alone tap the fused tap is compared with (tests/test_gpu_layouts.py::ROUTES: d64_immediate, wide80,
# chunk80_bf16)
STAND_ALONE = {('f16', 64): 'tap_d64_kernel', ('f16', 80): 'tap_wide_kernel', ('bf16', 64): 'tap_d64_kernel', ('bf16', 80): 'tap_chunk_kernel'}


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)


@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('hw', sd.HWS)
@pytest.mark.parametrize('d,heads', [(64, 2), (80, 4)])
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_attend_by_row_class(dt, d, heads, hw, accumulate, monkeypatch):
    """Output against ``ho.attention_output`` with the tolerances of tests/test_gpu_attend.py (fp16: test_attend_output_matches_reference,
    bf16: test_attend_bf16_pipeline) per row class; the fused tap's sums against the stand-alone tap of the same configuration (bit for
    bit where that file demands it, else its bf16 bound) and against the oracle like the tap routes above."""
    np_dt, dtype = (np.float16, torch.float16) if dt == 'f16' else (ho.BF16, torch.bfloat16)
    mode = f'{dt}_{"exact" if accumulate == "exact" else "f32acc"}'
    scale, n = d ** -0.5, 2
    steps, _ = _inputs(hw, heads, d, np_dt, n)
    values = sd.attend_values(hw, heads, d, np_dt, n)
    _configure(monkeypatch, {})
    fused, plain = _attend_engine(accumulate=accumulate), _attend_engine(accumulate=accumulate)
    what = f'attend {mode} d {d} hw {hw}'
    for s, ((q, k), v) in enumerate(zip(steps, values)):
        tq, tk, tv = _t(q, dtype), _t(k, dtype), _t(v, dtype)
        out = fused.attend(0, tq, tk, tv, heads, scale, 1, True, tapped=True)
        assert out is not None and out.shape == tq.shape and out.dtype == dtype, what
        # daam_attend records no kernel name; what can be told: the tap ran inside it (no tap launch on that context) ...
        assert fused.last_kernels(0) == '', (what, fused.last_kernels(0))
        plain.tap_qk(0, tq, tk, heads, scale, 1, True)
        assert plain.last_kernels(0) == STAND_ALONE[dt, d], (what, plain.last_kernels(0))      # ... and which kernel it is compared with
        qh, kh, vh = (sd.to_bh(np.asarray(x, np.float32), heads) for x in (q, k, v))
        want = np.asarray(ho.attention_output(qh, kh, vh, scale, np_dt), np.float64)          # [BATCH * heads, hw, d]
        got = sd.to_bh(out.float().cpu().numpy(), heads).astype(np.float64)
        assert np.isfinite(got).all(), what
        ref_scale = np.abs(want).max()
        err = np.abs(got - want)
        classes = sd.classify(sd.rounded_logits(qh, kh, scale, np_dt))                        # [BATCH * heads, hw]: every head has an output
        probs = np.asarray(ho.attention_probs(qh, kh, scale, np_dt), np.float64)
        tol, share = (2e-3 * ref_scale, 0.995) if dt == 'f16' else (2.0 ** -4 * ref_scale, 0.99)
        ulp = sd.ulp_of(want, np_dt)
        slack = sd.output_slack(probs, vh, np_dt)             # what one ulp on every probability of the row can move an output by
        within = err <= ulp
        report = {}
        for c, name in enumerate(sd.CLASS_NAMES):
            sel = classes == c
            assert sel.any(), (what, name)
            report[name] = (err[sel].max(), within[sel].mean(), (err[sel] / (ulp[sel] + slack[sel])).max())
        print(f'{what} step {s}: tolerance {tol:.3e}; (max-abs, share within one ulp, worst err / (ulp + slack)) per class -- {report}; '
              f'share of the call within one ulp {within.mean():.5f}')
        # the two tolerances of tests/test_gpu_attend.py: the largest error, per class, and the share of the call's elements within one ulp
        for name, (e, _, _) in report.items():
            assert e <= tol, f'{what} step {s} {name}: max-abs {e:.3e} (tolerance {tol:.3e})'
        assert within.mean() >= share, f'{what} step {s}: {within.mean():.4f} of the call within one ulp'
        # Per class the share is no property of a correct kernel: the project lets a probability be one ulp off (the fast exponential's
        # 1e-6 against the oracle's f32 softmax, tests/test_gpu_parity.py header), and that moves all head_dim outputs of the pixel by
        # ulp(p_t) |v_t| -- above the output's own ulp wherever the output is small by cancellation, which is most of an ``under`` row,
        # whose 77 tokens all carry probability (plain rows under a start-of-text token and one-token ``over`` rows hide it).  What does
        # hold per class, from the two number formats alone: every element within its own ulp plus one ulp on each probability of its row.
        # tests/test_softmax_domain_cpu.py::test_emulated_fast_softmax_* holds a numpy emulation of the fast softmax to the same checks:
        # on fp16, head_dim 80, hw 576, step 1 its ``under`` share is 0.99167 (one probability of 0.316 rounded the other way on the 34
        # identical ``under`` pixels of one level) and its worst err / (ulp + slack) 0.8826; the kernel measured the same two figures.
        for name, (_, _, worst) in report.items():
            assert worst <= 1.0, f'{what} step {s} {name}: an output {worst:.2f} x (its ulp + one ulp on every probability of its row) off'
        for name in ('plain', 'over'):                        # rows carried by a few tokens keep the share too
            assert report[name][1] >= share, f'{what} step {s} {name}: {report[name][1]:.4f} within one ulp'
    a, b = dict(fused.items()), dict(plain.items())
    assert list(a) == list(b) and len(a) == heads
    for key in a:
        assert a[key].dtype == b[key].dtype
        if dt == 'f16' or d <= 64:
            assert torch.equal(_bits(a[key]), _bits(b[key])), f'{what} {key}: fused and stand-alone tap differ'
        else:                                                 # bf16, head_dim > 64: another tiling (tests/test_gpu_attend.py::test_attend_bf16_pipeline)
            d2 = (a[key].float() - b[key].float()).abs()
            assert (d2 - (2.0 ** -3 * b[key].float().abs() + 2.0 ** -7)).max().item() <= 0 and (d2 > 0).float().mean().item() <= 0.01
    got = torch.stack([t for _, t in fused.items()]).float().cpu().numpy()
    acc_np = np.float32 if accumulate == 'float32' else np_dt
    want = _oracle(steps, heads, scale, np_dt, acc_np)
    pix = sd.pixel_classes(sd.row_classes(steps, heads, scale, np_dt))
    _assert_by_class(got, want, pix, _tolerance(mode, want, n), what + ' fused sums', sd.CLASS_NAMES)
    np.testing.assert_allclose(got.astype(np.float64).sum(-3), n, atol=n * 77 * (2.0 ** -8 if dt == 'bf16' else 2.0 ** -11))
    fused.close()
    plain.close()


# ---- the fp16 domain: |q.k| <= 65504 where the scale is a power of two ---------------------------------------------------------
IN_DOMAIN, OUT_OF_DOMAIN = 31.5, 32.0       # k of token 5 against q = 32 at head_dim 64: q.k = 64512 (logit 8064) / 65536 (logit 8192)
HOLE_HW = 256


def _hole_steps(d, heads, kval, n):
    """N(0,1) Q / K (Q rows minus their mean: token 5's constant K row then moves them by next to nothing); every fifth pixel has
    q = 32 in every component and token 5 has k = ``kval``: on those rows q.k of token 5 is ``32 * kval * d`` exactly (every partial
    sum is a multiple of 16 below 2^17), its logit is finite and representable in fp16, and every other token lies thousands below
    it: the row is 1 at token 5 and 0 elsewhere."""
    rng = np.random.default_rng([d, n, int(2 * kval)])
    steps = []
    for _ in range(n):
        q = rng.standard_normal((BATCH, HOLE_HW, heads, d))
        q = (q - q.mean(-1, keepdims=True)).astype(np.float16)
        k = rng.standard_normal((BATCH, sd.TOKENS, heads, d)).astype(np.float16)
        q[:, ::5] = np.float16(32.0)
        k[:, 5] = np.float16(kval)
        steps.append((q.reshape(BATCH, HOLE_HW, heads * d), k.reshape(BATCH, sd.TOKENS, heads * d)))
    return steps


def _hole_check(res_sums, steps, heads, d, what):
    want = _oracle(steps, heads, d ** -0.5, np.float16, np.float16)
    got = np.asarray(res_sums, np.float64)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite sums'
    classes = sd.pixel_classes(sd.row_classes(steps, heads, d ** -0.5, np.float16))
    assert (classes[:, ::5] == sd.OVER).all()
    _assert_by_class(got, want, classes, _tolerance('f16_exact', want, len(steps)), what, ('plain', 'over'))
    side = int(HOLE_HW ** 0.5)
    assert (got.reshape(-1, sd.TOKENS, side * side)[:, 5, ::5] == len(steps)).all(), what     # exactly 1 per step at token 5


# (route, mode, k of token 5): the largest in-domain value on every flavour; the first value outside on those that scale first
HOLE_CASES = [(r, 'f16_exact', IN_DOMAIN) for r in ('d64_deferred', 'd64_immediate', 'slab80', 'wide80', 'mfma')] + \
             [('d64_deferred', 'f16_strict', IN_DOMAIN), ('d64_deferred', 'f16_strict', OUT_OF_DOMAIN),
              ('mfma', 'f16_exact', OUT_OF_DOMAIN), ('slab80', 'f16_exact', OUT_OF_DOMAIN), ('wide80', 'f16_exact', OUT_OF_DOMAIN)]


@pytest.mark.parametrize('route,mode,kval', HOLE_CASES)
def test_fp16_logit_domain_tap(route, mode, kval, monkeypatch):
    spec = ROUTES[route]
    _, dtype, accumulate, env = MODES[mode]
    heads, d, n = spec['heads'], spec['d'], _n_steps(spec)
    steps = _hole_steps(d, heads, kval, n)
    _configure(monkeypatch, dict(spec['env'], **env))
    res = _tap_raw([(_dev(q), _dev(k)) for q, k in steps], heads, d, HOLE_HW, dtype, accumulate, 'L0', spec['deferred'])
    assert (res['name'], res['block']) == spec['kernel'], (res['name'], res['block'])
    _hole_check(res['sums'].float().numpy(), steps, heads, d, f'{route} {mode} k = {kval}')


@pytest.mark.parametrize('env,kval', [({}, IN_DOMAIN), (dict(DAAM_STRICT_EXP='1'), IN_DOMAIN), (dict(DAAM_STRICT_EXP='1'), OUT_OF_DOMAIN)],
                         ids=['fast_in_domain', 'strict_in_domain', 'strict_out_of_domain'])
def test_fp16_logit_domain_attend(env, kval, monkeypatch):
    heads, d, n = 2, 64, 2
    steps = _hole_steps(d, heads, kval, n)
    _configure(monkeypatch, env)
    eng = _attend_engine()
    rng = np.random.default_rng(3)
    for q, k in steps:
        v = rng.standard_normal((BATCH, sd.TOKENS, heads * d)).astype(np.float16)
        out = eng.attend(0, _dev(q), _dev(k), _dev(v), heads, 0.125, 1, True, tapped=True)
        assert out is not None and torch.isfinite(out).all()
        want = ho.attention_output(*(sd.to_bh(x, heads) for x in (q, k, v)), 0.125, np.float16).astype(np.float64)
        got = sd.to_bh(out.float().cpu().numpy(), heads).astype(np.float64)
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max()
        assert np.array_equal(got[:, ::5], want[:, ::5])                                      # those rows are V's row 5, bit for bit
    got = torch.stack([t for _, t in eng.items()]).float().cpu().numpy()
    eng.close()
    _hole_check(got, steps, heads, d, f'attend {env} k = {kval}')
