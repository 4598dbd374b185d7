"""Step protocol of the head_dim-64 tap (``tap_d64_kernel``): counted waits and one raw barrier per step (the default)
against the protocol before it (``DAAM_TAP_SYNC=0``: every DMA waited for, ``__syncthreads()``), against the four-wave form
(``DAAM_TAP_W8=0``), against the same steps tapped one launch each (no step follows another inside a launch there, so no K buffer is
reused and no Q tile refilled), and against the numpy oracle.

Shapes: heads 2, head_dim 64; hw 256 = one full eight-wave tile, 400 = a full tile and a partial one (wave 4 half inside: two of its
four Q pieces re-read piece 0's rows; waves 5..7 outside: they re-read the layer's last row), 1024 = four tiles per head.  The library
takes square maps only (``layer N holds M positions``), and no square is 8 pixels more than a multiple of 256 (a square that is a
multiple of 8 is a multiple of 16), so 400 stands for the "tile + 8 pixels" case.  Steps 1, 2, 3, 7, 50: both K buffers reused, odd and
even counts, the redundant re-fetch of the last step.  Every step has its own K whose start-of-sequence row is scaled differently, so
a K tile of step s - 1 or s + 1 in step s's place moves every sum far beyond an ulp."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import heatmap_oracle as ho
from test_gpu_parity import _dev, _engine, _qk, _to_bh

pytestmark = pytest.mark.gpu

HEADS, D, MAX_STEPS = 2, 64, 50
STEP_COUNTS = (1, 2, 3, 7, 50)
MODES = ['f16_exact', 'bf16_exact', 'f16_f32acc', 'f16_strict']
_inputs_cache, _oracle_cache = {}, {}


def _np_dtypes(mode):
    np_dt = ho.BF16 if mode.startswith('bf16') else np.float16
    return np_dt, (np.float32 if mode.endswith('_f32acc') else np_dt)


def _inputs(hw, np_dt):
    """50 (q, k) pairs, made once per (hw, dtype); K's start-of-sequence gain differs from step to step."""
    key = (hw, 'bf16' if ho.is_bf16(np_dt) else 'f16')
    if key not in _inputs_cache:
        rng = np.random.default_rng(hw * 7 + len(key[1]))
        _inputs_cache[key] = [_qk(rng, 2, HEADS, hw, D, np_dt, sos_gain=1.5 + 0.125 * s) for s in range(MAX_STEPS)]
    return _inputs_cache[key]


def _oracle(hw, mode):
    """{steps: sums after that many steps}: the reference's running sum, walked once per (hw, dtypes) and read at the step counts."""
    np_dt, acc_np = _np_dtypes(mode)
    key = (hw, 'f16_exact' if mode == 'f16_strict' else mode)   # the strict softmax is measured against the same reference
    if key not in _oracle_cache:
        raw, out = ho.RawMaps(acc_np), {}
        for s, (q, k) in enumerate(_inputs(hw, np_dt)):
            ho.tap(raw, 0, _to_bh(q, HEADS), _to_bh(k, HEADS), D ** -0.5, latent_hw=hw, pipe_dtype=np_dt)
            if s + 1 in STEP_COUNTS:
                out[s + 1] = np.stack([v for _, v in raw]).astype(np.float64)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _run(qk_dev, mode, defer):
    """Tap the steps on a fresh engine; returns (sums, block size, kernel names, steps of the last launch)."""
    eng = _engine(accumulate='float32' if mode.endswith('_f32acc') else 'exact', defer_steps=defer)
    for q, k in qk_dev:
        eng.tap_qk(0, q, k, HEADS, D ** -0.5, factor=1)
    got = torch.stack([v.float() for _, v in eng.items()]).cpu()
    grid, block, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    from daam_amd import _native as nat
    nat.check(eng.lib.daam_last_launch(eng.ctx, 0, ctypes.byref(grid), ctypes.byref(block), ctypes.byref(lds)))
    names, max_steps = eng.last_kernels(0), eng.last_flush()['max_steps']
    eng.close()
    return got, block.value, names, max_steps


@pytest.mark.parametrize('steps', STEP_COUNTS)
@pytest.mark.parametrize('hw', [256, 400, 1024])
@pytest.mark.parametrize('mode', MODES)
def test_counted_waits_keep_every_bit(mode, hw, steps, monkeypatch):
    from daam_amd import engine as E
    np_dt, _ = _np_dtypes(mode)
    qk_dev = [(_dev(q, np_dt), _dev(k, np_dt)) for q, k in _inputs(hw, np_dt)[:steps]]
    want = _oracle(hw, mode)[steps]

    def configure(**env):
        E.release_parked_contexts()                          # the switches are read when a native context is created
        for var in ('DAAM_TAP_SYNC', 'DAAM_TAP_W8', 'DAAM_STRICT_EXP'):
            monkeypatch.delenv(var, raising=False)
        if mode == 'f16_strict':
            monkeypatch.setenv('DAAM_STRICT_EXP', '1')
        for var, val in env.items():
            monkeypatch.setenv(var, val)

    configure()
    runs = [_run(qk_dev, mode, 64) for _ in range(3)]        # a race would not repeat itself
    got, block, names, launched = runs[0]
    assert launched == steps and block == 512 and names == 'tap_d64_kernel', (launched, block, names)
    for i, (g, b, n, _) in enumerate(runs[1:]):
        assert torch.equal(g, got) and (b, n) == (block, names), f'repetition {i + 1}: {(g != got).sum().item()} elements differ'
    each, _, n1, _ = _run(qk_dev, mode, 0)                     # every step a launch of its own
    assert n1 == 'tap_d64_kernel', n1
    assert torch.equal(got, each), f'deferred vs immediate: {(got != each).sum().item()} elements differ'
    configure(DAAM_TAP_SYNC='0')
    old, b_old, n_old, _ = _run(qk_dev, mode, 64)
    assert (b_old, n_old) == (512, 'tap_d64_kernel')
    assert torch.equal(got, old), f'counted vs DAAM_TAP_SYNC=0: {(got != old).sum().item()} elements differ'
    configure(DAAM_TAP_W8='0')
    four, b4, n4, _ = _run(qk_dev, mode, 64)
    assert (b4, n4) == (256, 'tap_d64_kernel')
    assert torch.equal(got, four), f'eight vs four waves: {(got != four).sum().item()} elements differ'
    configure()
    E.release_parked_contexts()

    # the 50-step tolerance of tests/test_gpu_parity.py::test_eight_wave_partial_tiles_50_deferred_steps_vs_oracle (written out in that
    # test's body, so it cannot be imported): an fp16 / bf16 running sum differs by an ulp of its magnitude a few times over the steps
    g = got.numpy().astype(np.float64)
    assert g.shape == want.shape
    ulp = 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11
    if mode.endswith('_f32acc'):
        tol = steps * ulp
    elif mode.startswith('bf16'):
        tol = 2.0 ** -4 * np.abs(want) + 2 * ulp * max(1.0, want.max())
    else:
        tol = 2.0 ** -6 * np.abs(want) + 2 * ulp * max(1.0, want.max())
    err = np.abs(g - want)
    print(f'{mode} hw {hw} steps {steps}: max-abs {err.max():.3e}')
    assert not (err > tol).any(), f'{mode} hw {hw} steps {steps}: {(err > tol).sum()} elements beyond tolerance, max-abs {err.max()}'
    np.testing.assert_allclose(g.sum(1), steps, atol=steps * 77 * ulp)      # every step's probabilities sum to one over the tokens
