"""The value side and the geometry of ``daam_attend`` against the numpy oracle in float64 accumulation (``tests/_attend_domain.py``
builds the inputs and derives the per-element bound; ``tests/test_attend_domain_cpu.py`` holds both to what this file relies on):

  1. value magnitudes   V whose small-probability tokens carry the output (``heavy_minor``), fp16-subnormal V (``tiny``), levels 2^-20
                        to 2^12 with cancelling signs (``mixed``), against rows whose minor probabilities are fp16 normals, subnormals,
                        single subnormal ulps and zeros; the fused tap's sums next to the stand-alone tap's and the oracle's
  2. every head dim     8, 16, .., 160: the zero-padded contraction and the cut last 16-row output tile of every ``AttendShape``
  3. cut tiles          pixel counts that cut a 128-pixel workgroup tile, a 32-pixel wave and a 16-pixel MFMA column group; fused taps on
                        rectangular layers (6 x 12, 13 x 16); pixel counts the predicate declines
  4. batch and heads    odd ``batch * heads``, batch 1 / 3 / 4, one head: which heads are kept

Every output element must lie inside ``ad.bound`` (its own ulp + one ulp on every probability of its row + an f32 accumulation in
another order); the worst ``err / bound`` per row kind is printed.  Outputs of tests 2 and 3 are also written through the raw ABI into
the middle of a sentinel-filled buffer: same bits, guards intact.  Run with ``-m gpu`` on an MI355X."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _attend_domain as ad
import _softmax_domain as sd
from oracle import heatmap_oracle as ho
from test_gpu_attend import _reference_eager
from test_gpu_layouts import DEV, _attend_desc, _bits, _configure
from test_gpu_softmax_domain import _tolerance

pytestmark = pytest.mark.gpu

DT = {'f16': (np.float16, torch.float16), 'bf16': (ho.BF16, torch.bfloat16)}
RECT = {136: (8, 17), 72: (6, 12), 208: (13, 16)}        # layers that are no squares: the map of a rectangular engine, factor 1
SENTINEL, GUARD = -7.0, 256                               # guard elements on either side of out (512 bytes: out stays 16-byte aligned)

_case_cache = {}


def _case(dt, d, heads, hw, v_set, n_steps, batch=2):
    """Inputs and oracle of a case, computed once: ``(steps [(q, k, v)], refs [ad.reference], kinds per pixel)``."""
    key = (dt, d, heads, hw, v_set, n_steps, batch)
    if key not in _case_cache:
        np_dt = DT[dt][0]
        qk, names = ad.build(hw, heads, d, np_dt, n_steps, batch)
        vs = ad.values(v_set, heads, d, np_dt, n_steps, batch)
        steps = [(q, k, v) for (q, k), v in zip(qk, vs)]
        _case_cache[key] = (steps, [ad.reference(q, k, v, heads, d ** -0.5, np_dt) for q, k, v in steps], names)
    return _case_cache[key]


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)      # exact: the values are the dtype's


def _engine(hw, accumulate='exact'):
    from daam_amd.engine import HeatMapEngine
    side = math.isqrt(hw)
    if side * side == hw:
        return HeatMapEngine(1, accumulate=accumulate, defer_steps=0), (side, side)
    return HeatMapEngine(1, accumulate=accumulate, defer_steps=0, out_hw=RECT[hw]), RECT[hw]


def _assert_inside_bound(out, ref, names, heads, what):
    got = sd.to_bh(out.float().cpu().numpy(), heads).astype(np.float64)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite outputs'
    worst = ad.worst_by_kind(got, ref, names)
    print(f'{what}: worst err / bound per kind -- {ad.report(worst)}')
    bad = {kind: (round(r, 3), at) for kind, (r, at) in worst.items() if r > 1.0}
    assert not bad, f'{what}: outside the bound at (head, pixel, element) -- {bad}'
    return worst


class _Contiguous:
    """Strides (batch, head, row) of a contiguous [B, rows, heads * d] tensor, as ``_attend_desc`` reads them."""

    def __init__(self, rows, heads, d):
        self.strides = (rows * heads * d, d, heads * d)


def _attend_into_guarded_buffer(eng, tq, tk, tv, heads, d, dtype):
    """The same call through the raw ABI with out in the middle of a sentinel-filled buffer: ``(out, guards intact)``."""
    from daam_amd import _native as nat
    b, hw, c = tq.shape
    assert b == 2                                             # _attend_desc: tests/test_gpu_layouts.py::BATCH
    n = tq.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + n].view(b, hw, c)
    assert out.data_ptr() % 16 == 0
    rows, keys = _Contiguous(hw, heads, d), _Contiguous(ad.TOKENS, heads, d)
    desc = _attend_desc(nat, dtype, heads, hw, d, rows, keys, keys, rows)
    nat.check(eng.lib.daam_attend(eng.ctx, 0, tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), out.data_ptr(), ctypes.byref(desc), 0, eng.stream))
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return out.clone(), intact


def _untapped(dt, d, heads, hw, v_set, monkeypatch, what):
    """One ``engine.attend`` call without the tap: shape, dtype, the bound on every element; the raw call's guards and bits."""
    _, dtype = DT[dt]
    steps, refs, names = _case(dt, d, heads, hw, v_set, 1)
    _configure(monkeypatch, {})
    eng, _ = _engine(256)
    tq, tk, tv = (_t(x, dtype) for x in steps[0])
    out = eng.attend(0, tq, tk, tv, heads, d ** -0.5, 1, True, tapped=False)
    assert out is not None, what
    assert out.shape == tq.shape and out.dtype == dtype, (what, out.shape, out.dtype)
    worst = _assert_inside_bound(out, refs[0], names, heads, what)
    again, intact = _attend_into_guarded_buffer(eng, tq, tk, tv, heads, d, dtype)
    eng.close()
    assert intact, f'{what}: a sentinel next to out was overwritten'
    assert torch.equal(_bits(again), _bits(out)), f'{what}: the raw call differs from engine.attend'
    return worst


def _tapped(dt, d, heads, hw, v_set, accumulate, monkeypatch, what, batch=2, n_steps=2):
    """``n_steps`` ``engine.attend`` calls with the fused tap, the same steps through ``tap_qk`` on a second engine: outputs inside the
    bound; the sums' keys, dtype and bits (bf16 above head_dim 64: the bound of tests/test_gpu_attend.py::test_attend_bf16_pipeline)
    against the stand-alone tap; the sums against the oracle with the tolerance of tests/test_gpu_parity.py::test_tap_qk_vs_oracle."""
    np_dt, dtype = DT[dt]
    scale = d ** -0.5
    steps, refs, names = _case(dt, d, heads, hw, v_set, n_steps, batch)
    _configure(monkeypatch, {})
    (fused, (h, w)), (plain, _) = _engine(hw, accumulate), _engine(hw, accumulate)
    total = {}
    for s, ((q, k, v), ref) in enumerate(zip(steps, refs)):
        tq, tk, tv = _t(q, dtype), _t(k, dtype), _t(v, dtype)
        out = fused.attend(0, tq, tk, tv, heads, scale, 1, True, tapped=True)
        assert out is not None and out.shape == tq.shape and out.dtype == dtype, what
        assert fused.last_kernels(0) == '', (what, fused.last_kernels(0))      # the tap ran inside daam_attend: no tap launch of its own
        plain.tap_qk(0, tq, tk, heads, scale, 1, True)
        for kind, (r, _) in _assert_inside_bound(out, ref, names, heads, f'{what} step {s}').items():
            total[kind] = max(total.get(kind, 0.0), r)
        # the reference's torch ops in eager: reported only (whether its GEMM keeps fp16-subnormal probabilities is not known)
        eager = sd.to_bh(_reference_eager(tq, tk, tv, heads, scale)[0].float().cpu().numpy(), heads).astype(np.float64)
        small = np.isin(names, ('gap12', 'gap16'))
        print(f'{what} step {s}: eager reference vs oracle on the gap12 / gap16 rows, worst |diff| / bound '
              f'{(np.abs(eager - ref["want"]) / ref["bound"])[:, small].max():.3f}; stand-alone tap: {plain.last_kernels(0)}')
    a, b = dict(fused.items()), dict(plain.items())
    bh = batch * heads
    assert list(a) == list(b) and len(a) == bh - bh // 2, (what, list(a), list(b))
    for key in a:
        assert a[key].dtype == b[key].dtype == (torch.float32 if accumulate == 'float32' else dtype), (what, key)
        assert tuple(a[key].shape) == (ad.TOKENS, h, w), (what, key, a[key].shape)
        if dt == 'f16' or d <= 64:
            assert torch.equal(_bits(a[key]), _bits(b[key])), f'{what} {key}: fused and stand-alone tap differ'
        else:
            d2 = (a[key].float() - b[key].float()).abs()
            assert (d2 - (2.0 ** -3 * b[key].float().abs() + 2.0 ** -7)).max().item() <= 0 and (d2 > 0).float().mean().item() <= 0.01
    got = torch.stack([t for _, t in fused.items()]).float().cpu().numpy().astype(np.float64)
    fused.close()
    plain.close()
    # the kept heads are [BH // 2, BH) (trace.py:240), one add per step in the sum dtype
    want = ad.rect_sums([ref['probs'] for ref in refs], np.float32 if accumulate == 'float32' else np_dt, h, w)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = _tolerance(f'{dt}_{"exact" if accumulate == "exact" else "f32acc"}', want, n_steps)
    err = np.abs(got - want).max()
    print(f'{what}: fused sums vs oracle max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{what}: fused sums {err:.3e} beyond {tol:.3e}'
    half_ulp = 2.0 ** -8 if dt == 'bf16' else 2.0 ** -11
    np.testing.assert_allclose(got.sum(-3), n_steps, atol=n_steps * 77 * half_ulp, err_msg=what)
    return total


# ---- 1. value sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('v_set', ad.V_SETS)
@pytest.mark.parametrize('hw', [256, 136])
@pytest.mark.parametrize('d,heads', [(64, 2), (80, 4)])
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_value_sets(dt, d, heads, hw, v_set, accumulate, monkeypatch):
    """The gap12 / gap16 rows of ``heavy_minor`` are where an fp16-subnormal probability that the second product dropped would show
    (tests/test_attend_domain_cpu.py::test_dropped_subnormal_probabilities_are_visible: 36 to 60 x the bound): held against the
    numpy oracle only."""
    worst = _tapped(dt, d, heads, hw, v_set, accumulate, monkeypatch, f'values {dt} d {d} hw {hw} {v_set} {accumulate}')
    assert set(worst) == set(ad.KIND_NAMES)


# ---- 2. every head dim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', ad.HEAD_DIMS)
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_every_head_dim(dt, d, monkeypatch):
    worst = _untapped(dt, d, 3, 136, 'mixed', monkeypatch, f'head_dim {dt} d {d} hw 136 mixed')
    assert set(worst) == set(ad.KIND_NAMES)


# ---- 3. cut tiles ----------------------------------------------------------------------------------------------------------------
CUT_HWS = (8, 24, 40, 120, 136, 208, 264)
CUT_SHAPES = [('f16', 40), ('f16', 64), ('f16', 160), ('bf16', 64)]


@pytest.mark.parametrize('v_set', ['plain', 'heavy_minor'])
@pytest.mark.parametrize('hw', CUT_HWS)
@pytest.mark.parametrize('dt,d', CUT_SHAPES)
def test_cut_tiles(dt, d, hw, v_set, monkeypatch):
    """8 = half a column group; 24 = a group and a half; 40 = a wave and a half group; 120 = a workgroup tile less half a group;
    136 / 264 = one / two tiles and half a group; 208 = a tile, two waves and a group."""
    worst = _untapped(dt, d, 2, hw, v_set, monkeypatch, f'cut {dt} d {d} hw {hw} {v_set}')
    assert set(worst) == set(ad.KIND_NAMES)


@pytest.mark.parametrize('hw', [72, 208])
@pytest.mark.parametrize('dt,d', CUT_SHAPES)
def test_cut_tiles_with_the_fused_tap_on_a_rectangular_layer(dt, d, hw, monkeypatch):
    """6 x 12 and 13 x 16 layers on a rectangular engine: the sums' rows are 72 / 208 pixels long, so the 16-byte pieces of the last
    column groups end inside the tile; ``[kept heads, 77, h, w]`` against the oracle."""
    _tapped(dt, d, 2, hw, 'heavy_minor', 'exact', monkeypatch, f'rect tap {dt} d {d} hw {hw}')


@pytest.mark.parametrize('hw', [20, 988])
def test_pixel_counts_that_are_no_multiple_of_8_are_declined(hw, monkeypatch):
    """The fused tap updates the sums in 16-byte row pieces: ``hw % 8 != 0`` is outside the predicate (988 = 26 x 38, an SD-v1.5 layer
    of a 208 x 304 generation)."""
    _, dtype = DT['f16']
    (q, k), = ad.build(hw, 2, 64, np.float16, 1)[0]
    v, = ad.values('plain', 2, 64, np.float16, 1)
    _configure(monkeypatch, {})
    eng, _ = _engine(256)
    for tapped in (False, True):
        assert eng.attend(0, _t(q, dtype), _t(k, dtype), _t(v, dtype), 2, 0.125, 1, True, tapped=tapped) is None
    assert not list(eng.items())
    eng.close()


# ---- 4. batch and heads splits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch,heads', [(1, 4), (1, 3), (3, 3), (4, 2), (2, 1)])
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_batch_and_heads_splits(dt, batch, heads, monkeypatch):
    """No CFG (batch 1: the kept heads start inside the only batch element), an odd ``batch * heads`` (3, 9: the kept half is the larger
    one), batch 4, one head per batch element.  Every one of the ``batch * heads`` outputs is checked; the kept sums are the oracle's
    heads ``[BH // 2, BH)``."""
    worst = _tapped(dt, 64, heads, 136, 'heavy_minor', 'exact', monkeypatch, f'split {dt} batch {batch} heads {heads}', batch=batch)
    assert set(worst) == set(ad.KIND_NAMES)
