"""Finalize kernels, token row by token row, across plane magnitudes: every finalize route against the float64 oracle on "levelled
planes" (``tests/_finalize_domain.py``: token rows up to 2^21 apart, the whole set scaled by 2^k), each token row measured against ITS
OWN maximum.  One absolute bound over all 77 rows -- what ``test_gpu_parity.py`` uses on planes of magnitude 3 -- sees neither a 1e-5
leak of the start-of-text row into a content row nor an error floor that does not shrink with the values.

Contracts (derived in ``_finalize_domain.py``):  exact-f32 routes ``err_t <= 2^-19 * rowmax_t``;  MFMA x2 routes, planes inside
``|v| <= 2^15``, ``err_t <= 2^-19 * rowmax_t + 2^-23``.  Every case asserts through ``last_kernels(1)`` which kernels ran.

What an MI355X gave is in LABNOTES.md (R7.3); run with ``-s``, every case prints one ``FINDOMAIN`` line with its figures.
"""
import math
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

import _finalize_domain as fd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TAG = {'float16': 'f16', 'bfloat16': 'bf16', 'float32': 'f32'}
ROUTES = {
    'default': {},
    'no_fold': {'DAAM_NO_FOLD_SAME': '1'},
    'no_pipe': {'DAAM_NO_PIPE_FINALIZE': '1'},
    'no_mfma': {'DAAM_NO_MFMA_FINALIZE': '1'},
    'general': {'DAAM_FORCE_GENERIC': '1'},
}
_SWITCHES = ('DAAM_NO_FOLD_SAME', 'DAAM_NO_PIPE_FINALIZE', 'DAAM_NO_MFMA_FINALIZE', 'DAAM_FORCE_GENERIC')


def _set_route(monkeypatch, route):
    for name in _SWITCHES:                                       # read when the native context is created
        monkeypatch.setenv(name, ROUTES[route].get(name, '0'))


def _ids(sides):
    return 'x'.join(map(str, sides))


def expected_kernels(sides, dtype, route, grouped=False):
    """``(kernel names one finalize call must launch, does the x2 class run on an MFMA kernel)`` for layers of ``sides`` with equal head
    counts: the planner's rules (csrc/daam_finalize_api.hip, fin_plan / fin_single) restated."""
    tag, out_side, g = TAG[dtype], fd.out_side_of(sides), '_grouped' if grouped else ''
    if route == 'general':
        return {f'finalize{g}_kernel<{tag}>'}, False
    names, mfma = set(), False
    same = out_side in sides
    x2 = 32 in sides and out_side == 64
    x2_kernel = None
    if x2:
        if route == 'no_mfma' or (route == 'no_pipe' and dtype != 'float16'):
            x2_kernel = f'finalize_up{g}_kernel<32><{tag}>'
        elif route == 'no_pipe':
            assert not grouped
            mfma = True
            x2_kernel = 'finalize_up32_same_kernel<f16>' if same else 'finalize_up32_mfma_kernel<f16>'
            same = False                                         # the paired kernel takes the same-size class along
        else:
            mfma = True
            fold = same and route != 'no_fold'
            x2_kernel = f'finalize_up32_pipe{g}_kernel<{tag}' + (' + same-size keys>' if fold else '>')
            same = same and not fold
        names.add(x2_kernel)
    if same:
        names.add(f'finalize_same{g}_kernel<{tag}>')
    for side in sides:
        if side in (32, out_side):
            continue
        if out_side == 64 and side == 16:
            names.add(f'finalize_up{g}_kernel<16><{tag}>')
        elif out_side == 64 and side == 128:
            names.add(f'finalize_down2{g}_kernel<{tag}>')
        else:
            names.add(f'finalize{g}_kernel<{tag}>')
    return names, mfma


def _launched(eng):
    return set(re.split(r'\+(?![^<]*>)', eng.last_kernels(1)))   # '+' between kernels, not the one inside <...>


def _dev(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(torch.bfloat16) if dtype == 'bfloat16' else t


def _engine(sides, dtype, **kw):
    from daam_amd.engine import HeatMapEngine
    return HeatMapEngine(len(sides), tokens=fd.TOKENS, out_side=fd.out_side_of(sides),
                         accumulate='float32' if dtype == 'float32' else 'exact', **kw)


def _tap(eng, planes, sides, dtype):
    out_side = fd.out_side_of(sides)
    for layer, (side, p) in enumerate(zip(sides, planes)):
        eng.tap_probs(layer, _dev(p, dtype), factor=fd.factor_of(side, out_side))


def _finalize(planes, sides, dtype):
    eng = _engine(sides, dtype)
    _tap(eng, planes, sides, dtype)
    got = eng.global_heat_map().cpu().numpy()
    names = _launched(eng)
    eng.close()
    return got, names


@lru_cache(maxsize=None)
def _base(sides, variant, heads=fd.HEADS):
    return fd.draw_planes(sides, variant, heads)


@lru_cache(maxsize=None)
def _reference0(sides, dtype, variant):
    """The float64 oracle of the k = 0 planes rounded to ``dtype``: computed once, shared by the five routes and every k, never changed."""
    want = fd.reference64([fd.round_to(b, dtype) for b in _base(sides, variant)], sides, fd.out_side_of(sides))
    want.setflags(write=False)
    return want


def _report(what, names, rel, ab):
    """One line per case for the record (``fd.worst``: on an MFMA route the ratio is over the rows of the relative regime, the
    absolute error over the rows of the floor regime)."""
    print(f'\nFINDOMAIN {what} | {"+".join(sorted(names))} | err_t/rowmax_t <= 2^{math.log2(max(rel, 1e-300)):.2f} | '
          f'err_t <= 2^{math.log2(max(ab, 1e-300)):.2f}')


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('dtype', fd.DTYPES)
@pytest.mark.parametrize('sides', fd.SIDES, ids=_ids)
def test_levelled_planes_vs_float64(sides, dtype, route, monkeypatch):
    """Every class / side of ``test_finalize_vs_oracle`` x the sums' dtypes x the five routes, non-negative and signed, at every k of
    the route's list.  Exact routes: k in {-20, -10, 0, 6, 12} and 40 for bf16 / f32 sums; MFMA x2 routes: {-10, 0, 6, 12}.  Where the planes
    must stay inside 2^15 (the MFMA routes' domain; fp16 sums hold no more than 65504 on any route) the draw is divided by a power of two: a
    requested 12 becomes 7 or 8."""
    _set_route(monkeypatch, route)
    want_names, mfma = expected_kernels(sides, dtype, route)
    ks = fd.K_MFMA if mfma else fd.K_EXACT + ([40] if dtype != 'float16' else [])
    limit = fd.DOMAIN_MAX if mfma or dtype == 'float16' else None
    out_side = fd.out_side_of(sides)
    worst_rel = worst_abs = 0.0
    for variant in fd.VARIANTS:
        base = _base(sides, variant)
        for k in ks:
            k = fd.scale_exp(base, k, limit)
            planes, homogeneous = fd.scaled_planes(base, k, dtype)
            assert all(np.isfinite(p.astype(np.float32)).all() for p in planes)
            # bicubic, clamp and mean are positively homogeneous: the k = 0 reference times 2^k, unless the cast changed a value
            want = _reference0(sides, dtype, variant) * 2.0 ** k if homogeneous else fd.reference64(planes, sides, out_side)
            got, names = _finalize(planes, sides, dtype)
            assert names == want_names, (names, want_names)
            rel, ab = fd.assert_contract(got, want, mfma, f'{_ids(sides)} {dtype} {route} {variant} k={k}')
            worst_rel, worst_abs = max(worst_rel, rel), max(worst_abs, ab)
    _report(f'matrix {_ids(sides)} {dtype} {route} mfma={int(mfma)}', want_names, worst_rel, worst_abs)


def _two_group_planes(variant, dtype, seed):
    """Sides (32, 64), four kept heads per layer = two prompts of two; group 1 (heads 2, 3) is 2^-10 of group 0: a leak of group 0
    into group 1 is 2^10 times what the same leak between equals would be."""
    sides = (32, 64)
    base = fd.draw_planes(sides, variant, heads=4, seed=seed)
    for b in base:
        b[6:] *= np.float32(2.0 ** -10)                           # [4 zero heads | group 0: 4, 5 | group 1: 6, 7]
    planes = [fd.round_to(b, dtype) for b in base]
    halves = [[np.concatenate([p[:2], p[4 + 2 * g:6 + 2 * g]]) for p in planes] for g in range(2)]   # [2 zero | 2 kept] per group
    return sides, planes, halves


@pytest.mark.parametrize('variant', fd.VARIANTS)
@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_groups_levelled(dtype, variant, monkeypatch):
    """``daam_finalize_groups`` (two prompts of one batched generation) on the grouped pipelined kernel, k = 0."""
    _set_route(monkeypatch, 'default')
    sides, planes, halves = _two_group_planes(variant, dtype, seed=1)
    eng = _engine(sides, dtype)
    _tap(eng, planes, sides, dtype)
    got = eng.global_heat_maps(2, [fd.TOKENS, fd.TOKENS]).cpu().numpy()
    want_names, mfma = expected_kernels(sides, dtype, 'default', grouped=True)
    assert _launched(eng) == want_names and mfma, eng.last_kernels(1)
    eng.close()
    for g in range(2):
        rel, ab = fd.assert_contract(got[g], fd.reference64(halves[g], sides, 64), True, f'groups {dtype} {variant} group {g}')
        _report(f'groups {dtype} {variant} group {g} mfma=1', want_names, rel, ab)


@pytest.mark.parametrize('variant', fd.VARIANTS)
@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_time_bins_levelled(dtype, variant, monkeypatch):
    """A context of two time windows, ``time_heat_maps`` (``daam_finalize_bins``): single windows straight on the windows' planes (grouped
    pipelined kernel of the sums' dtype), and the window range [0, 2) through the f32 window sum (grouped pipelined kernel on f32 planes)."""
    _set_route(monkeypatch, 'default')
    steps = [_two_group_planes(variant, dtype, seed=2 + s) for s in range(2)]
    sides = steps[0][0]
    eng = _engine(sides, dtype, time_bins=[0, 1])
    for _, planes, _ in steps:                                   # step s of every layer lands in window s
        _tap(eng, planes, sides, dtype)
    pipe = 'finalize_up32_pipe_grouped_kernel<%s + same-size keys>'
    got = eng.time_heat_maps([(0, 1, 0), (1, 2, 1)], 2, [fd.TOKENS, fd.TOKENS]).cpu().numpy()
    assert _launched(eng) == {pipe % TAG[dtype]}, eng.last_kernels(1)
    for g in range(2):                                           # (window g, prompt g)
        rel, ab = fd.assert_contract(got[g], fd.reference64(steps[g][2][g], sides, 64), True, f'bins {dtype} {variant} window {g}')
        _report(f'bins single window {dtype} {variant} group {g} mfma=1', _launched(eng), rel, ab)
    got = eng.time_heat_maps([(0, 2, 0), (0, 2, 1)], 2, [fd.TOKENS, fd.TOKENS]).cpu().numpy()
    assert _launched(eng) == {f'finalize_bin_sum_kernel<{TAG[dtype]}>', pipe % 'f32'}, eng.last_kernels(1)
    for g in range(2):
        summed = [a.astype(np.float64) + b.astype(np.float64) for a, b in zip(steps[0][2][g], steps[1][2][g])]
        rel, ab = fd.assert_contract(got[g], fd.reference64(summed, sides, 64), True, f'bins {dtype} {variant} range, prompt {g}')
        _report(f'bins window range {dtype} {variant} group {g} mfma=1', _launched(eng), rel, ab)
    eng.close()


MFMA_ROUTES = [(r, d) for r in ('default', 'no_fold') for d in fd.DTYPES] + [('no_pipe', 'float16')]


@pytest.mark.parametrize('with_same', [False, True], ids=['x2_only', 'with_same_size_layer'])
@pytest.mark.parametrize('token', [1, 38, 76])
@pytest.mark.parametrize('route,dtype', MFMA_ROUTES)
def test_no_leak_between_token_rows(route, dtype, token, with_same, monkeypatch):
    """Token 0 at level 2^6, one content token at 2^-9, every other token row exactly zero, on three x2 keys (the pointer table pads
    them with a zero plane) and, ``with_same``, two same-size keys riding along: the zero rows come out exactly 0.0 -- whatever reaches them
    came from another token's plane (ring slot, table padding, a race) -- and the two live rows meet the contract."""
    _set_route(monkeypatch, route)
    sides = (32, 64) if with_same else (32,)
    rng = np.random.default_rng([7, token, int(with_same)])
    planes = []
    for side, heads in zip(sides, (3, 2)):
        x = np.zeros((heads, side * side, fd.TOKENS), np.float32)
        x[..., 0] = np.exp(rng.standard_normal(x.shape[:2])) * 2.0 ** 6
        x[..., token] = np.exp(rng.standard_normal(x.shape[:2])) * 2.0 ** -9
        planes.append(fd.round_to(np.concatenate([np.zeros_like(x), x]), dtype))
    assert max(float(np.abs(p.astype(np.float32)).max()) for p in planes) <= fd.DOMAIN_MAX
    want = fd.reference64(planes, sides, 64)
    got, names = _finalize(planes, sides, dtype)
    want_names, mfma = expected_kernels(sides, dtype, route)
    assert names == want_names and mfma, (names, want_names)
    zero_rows = [t for t in range(fd.TOKENS) if t not in (0, token)]
    assert not want[zero_rows].any()
    leaked = np.abs(got[zero_rows]).reshape(len(zero_rows), -1).max(1)
    assert (got[zero_rows] == 0.0).all(), \
        f'{route} {dtype}: zero token rows hold up to {leaked.max():.3e} (rows {[zero_rows[i] for i in np.nonzero(leaked)[0][:8]]})'
    rel, ab = fd.assert_contract(got, want, True, f'leak probe {route} {dtype} token {token}')
    _report(f'leak probe {route} {dtype} token {token} same={int(with_same)} mfma=1', names, rel, ab)


@pytest.mark.parametrize('route', ['default', 'no_mfma'])
@pytest.mark.parametrize('sides', [(32,), (32, 64)], ids=_ids)
def test_fp16_subnormal_planes(sides, route, monkeypatch):
    """fp16 sums whose every element is an fp16 subnormal, m * 2^-24 with m in [1, 511] (so within [2^-24, 2^-15)): exact numbers for the
    oracle.  The LDS route meets the relative contract; the MFMA route its contract with the 2^-23 floor -- were subnormal inputs of
    ``v_mfma_f32_32x32x16_f16`` flushed to zero, the error would be the values themselves, about 2^-15."""
    _set_route(monkeypatch, route)
    rng = np.random.default_rng([11, len(sides)])
    planes = []
    for side in sides:
        x = (rng.integers(1, 512, (fd.HEADS, side * side, fd.TOKENS)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float16)
        assert (x > 0).all() and (x < np.float16(2.0 ** -14)).all()
        planes.append(np.concatenate([np.zeros_like(x), x]))
    want = fd.reference64(planes, sides, 64)
    got, names = _finalize(planes, sides, 'float16')
    want_names, mfma = expected_kernels(sides, 'float16', route)
    assert names == want_names and mfma == (route == 'default'), (names, want_names)
    err, rowmax = fd.row_errors(got, want)
    print(f'\nFINDOMAIN subnormal {_ids(sides)} {route} mfma={int(mfma)} | {"+".join(sorted(names))} | err_t <= 2^{math.log2(max(err.max(), 1e-300)):.2f}'
          f' | rowmax_t >= 2^{math.log2(rowmax.min()):.2f} | err_t/rowmax_t <= 2^{math.log2(max((err / rowmax).max(), 1e-300)):.2f}')
    fd.assert_contract(got, want, mfma, f'fp16 subnormal planes {_ids(sides)} {route}')
