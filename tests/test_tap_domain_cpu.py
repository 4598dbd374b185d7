"""The inputs, the reference and the bound of ``tests/test_gpu_tap_domain.py`` hold what that file relies on (no GPU): the logits do
not depend on the summation order, the row kinds are what their names say, the literal oracle and a numpy emulation of the kernels'
fast softmax stay inside the per-probability bound and pass the bias rule, and each of the five mutants of ``tests/_tap_domain.py``
fails the assertion named for it -- the subnormal flush while it PASSES the tolerance every earlier tap test uses."""
import numpy as np
import pytest

import _attend_domain as ad
import _softmax_domain as sd
import _tap_domain as td
from oracle import heatmap_oracle as ho

DTYPES = {'f16': np.float16, 'bf16': ho.BF16}
HEADS = {40: 8, 64: 2, 80: 4, 160: 2}                # as the routes of tests/test_gpu_layouts.py
HWS = (256, 576)
SUBNORMAL_MIN = 2.0 ** -24

_cache = {}


def _case(dt, d, hw, n_steps, accumulate, upcast=False):
    """``(steps, names, reference)``, computed once."""
    np_dt = DTYPES.get(dt, np.float32)
    key = (dt, d, hw, n_steps)
    if key not in _cache:
        _cache[key] = ad.build(hw, HEADS[d], d, np_dt, n_steps)
    steps, names = _cache[key]
    rkey = key + (accumulate, upcast)
    if rkey not in _cache:
        _cache[rkey] = td.reference(steps, HEADS[d], d ** -0.5, np_dt, td.sum_dtype(np_dt, accumulate), upcast)
    return steps, names, _cache[rkey]


@pytest.mark.parametrize('dt,upcast', [('f16', False), ('bf16', False), ('f16', True), ('f32', False)])
@pytest.mark.parametrize('d', sorted(HEADS))
def test_no_logit_depends_on_the_summation_order(d, dt, upcast):
    """Reversing the head_dim axis of Q and K changes no logit: rounded to the pipeline dtype, unrounded (``round_logits = 0``) or f32."""
    np_dt, scale = DTYPES.get(dt, np.float32), d ** -0.5
    steps, _ = ad.build(256, HEADS[d], d, np_dt, 2)
    for q, k in steps:
        qh, kh = (sd.kept(sd.to_bh(np.asarray(x, np.float32), HEADS[d])) for x in (q, k))
        qr, kr = np.ascontiguousarray(qh[..., ::-1]), np.ascontiguousarray(kh[..., ::-1])
        np.testing.assert_array_equal(sd.rounded_logits(qh, kh, scale, np_dt, upcast), sd.rounded_logits(qr, kr, scale, np_dt, upcast))


@pytest.mark.parametrize('d', sorted(HEADS))
def test_every_kind_is_present_and_is_what_its_name_says(d):
    """hw 256 has every kind; on the float64 softmax of the fp16 logits the gap rows' minor probabilities are fp16 normals (gap8),
    fp16 subnormals of at least one ulp (gap12), half an ulp to 32 ulps (gap16: none rounds to zero) and below half an ulp (gap20)."""
    steps, names, ref = _case('f16', d, 256, 3, 'exact')
    assert set(names) == set(ad.KIND_NAMES)
    for s, p64 in enumerate(ref['p64']):
        for kind, (lo, hi) in dict(gap8=(td.NORMAL_MIN, 2.0 ** -7), gap12=(SUBNORMAL_MIN, td.NORMAL_MIN),
                                   gap16=(SUBNORMAL_MIN / 2, 32.5 * SUBNORMAL_MIN), gap20=(0.0, SUBNORMAL_MIN / 2)).items():
            rows = np.nonzero(names == kind)[0]
            minor = np.stack([p64[:, p][:, np.arange(ad.TOKENS) != ad.designed_token(p, s)] for p in rows], 1)
            assert (minor > lo).all() and (minor < hi).all(), (kind, s, minor.min(), minor.max())
            assert {ad.designed_token(p, s) for p in rows} == set(ad.DESIGNED)
    # the rotation: over three steps an element of a designed token receives a probability near 1 and one below 2^-14
    lead = td.per_token(ref['p64'].max(0))[:, list(ad.DESIGNED)][..., names == 'gap16']
    least = td.per_token(ref['p64'].min(0))[:, list(ad.DESIGNED)][..., names == 'gap16']
    assert ((lead > 0.99) & (least < td.NORMAL_MIN)).any()


@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('d', sorted(HEADS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_oracle_and_emulation_are_inside_the_bound(dt, d, hw):
    """``ho.tap`` into ``ho.RawMaps`` and ``sd.emulate_fast_probs`` + the sum, three steps, both sum dtypes: every element within E_n,
    and on the f32 sums the rounding bias within 0.05 ulp."""
    np_dt = DTYPES[dt]
    for accumulate in ('exact', 'float32'):
        steps, names, ref = _case(dt, d, hw, 3, accumulate)
        acc_np = td.sum_dtype(np_dt, accumulate)
        what = f'{dt} d {d} hw {hw} {accumulate}'
        got = {'oracle': td.oracle_sums(steps, HEADS[d], d ** -0.5, np_dt, acc_np),
               'emulation': td.emulated_sums(ref['logits'], np_dt, acc_np, names)}
        for who, sums in got.items():
            td.assert_inside_bound(sums, ref, names, f'{who} {what}')
            if accumulate == 'float32':
                td.assert_unbiased(sums, ref, names, np_dt, f'{who} {what}')


def test_the_hooked_emulation_is_the_emulation():
    _, _, ref = _case('f16', 64, 256, 2, 'exact')
    for np_dt in DTYPES.values():
        np.testing.assert_array_equal(td.emulated_probs(ref['logits'][0], np_dt), sd.emulate_fast_probs(ref['logits'][0], np_dt))


def test_the_smallest_case_carries_the_bias_rule():
    """hw 256 with two kept heads: 6158 elements of ``spread`` pixels are fp16 normals -- above the 4096 the rule's sigma needs."""
    _, names, ref = _case('f16', 64, 256, 1, 'float32')
    _, count = td.bias(td.per_token(ref['p64'][0]), ref, names, np.float16)
    assert count == 6158


@pytest.mark.parametrize('hw', HWS)
def test_oracle_is_inside_the_bound_with_unrounded_logits_and_in_f32(hw):
    """``round_logits = 0`` (upcast_attention) on fp16, and the f32 pipeline with its ``c`` read off ``tap_generic_kernel``."""
    steps, names, ref = _case('f16', 64, hw, 2, 'exact', upcast=True)
    td.assert_inside_bound(td.oracle_sums(steps, 2, 0.125, np.float16, np.float16, upcast=True), ref, names, f'oracle upcast hw {hw}')
    steps, names, ref = _case('f32', 64, hw, 2, 'exact')
    worst = td.assert_inside_bound(td.oracle_sums(steps, 2, 0.125, np.float32, np.float32), ref, names, f'oracle f32 hw {hw}')
    # ... and that bound is an f32 one, relative to every element: c + 2 < 256
    assert (ref['bound'] <= 2.0 ** -16 * ref['want']).all() and max(r for r, _ in worst.values()) > 0.0


def _mutant(dt, d, mutant, n_steps, accumulate, hw=256):
    np_dt = DTYPES[dt]
    _, names, ref = _case(dt, d, hw, n_steps, accumulate)
    return td.emulated_sums(ref['logits'], np_dt, td.sum_dtype(np_dt, accumulate), names, mutant), ref, names


@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('d', sorted(HEADS))
def test_mutant_flush_fails_the_bound_and_passes_the_old_tolerance(d, accumulate):
    """fp16 probabilities below 2^-14 set to zero: 100 ulps out on the gap12 rows, yet inside ``2 half_ulp max(1, max want)`` /
    ``steps half_ulp`` -- the gap this file closes, pinned."""
    for n in (2, 3):
        got, ref, names = _mutant('f16', d, 'flush', n, accumulate)
        worst = td.worst_by_kind(got, ref, names)
        old = np.abs(got - ref['want']).max() / td.old_tolerance(np.float16, td.sum_dtype(np.float16, accumulate), ref['want'], n)
        print(f'flush d {d} {accumulate} {n} steps: {td.report(worst)}; {old:.3f} of the old tolerance')
        assert worst['gap12'][0] >= 10.0 and worst['gap16'][0] > 1.0, worst
        assert old <= 1.0, old
        with pytest.raises(AssertionError, match='outside the bound'):
            td.assert_inside_bound(got, ref, names, 'flush')


@pytest.mark.parametrize('d', sorted(HEADS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_mutant_truncate_fails_the_bias_rule_only(dt, d):
    """A conversion that rounds toward zero stays inside one ulp of every probability; its mean error is half an ulp."""
    for n in (2, 3):
        got, ref, names = _mutant(dt, d, 'truncate', n, 'float32')
        td.assert_inside_bound(got, ref, names, f'truncate {dt} d {d} {n} steps')
        mean, count = td.bias(got, ref, names, DTYPES[dt])
        print(f'truncate {dt} d {d} {n} steps: bias {mean:+.4f} over {count}')
        assert -0.52 <= mean <= -0.48 and count >= td.BIAS_MIN_COUNT
        with pytest.raises(AssertionError, match='does not round to nearest'):
            td.assert_unbiased(got, ref, names, DTYPES[dt], 'truncate')


@pytest.mark.parametrize('mutant,kind', [('swap', 'gap8'), ('padding', 'spread')])
@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('d', sorted(HEADS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_mutants_swap_and_padding_fail_the_bound(dt, d, accumulate, mutant, kind):
    """Two minor tokens exchanged on the gap rows; three un-masked padding slots in the row sum (4 % of a ``spread`` row's sum)."""
    for n in (2, 3):
        got, ref, names = _mutant(dt, d, mutant, n, accumulate)
        worst = td.worst_by_kind(got, ref, names)
        print(f'{mutant} {dt} d {d} {accumulate} {n} steps: {td.report(worst)}')
        assert worst[kind][0] >= 4.0, worst
        with pytest.raises(AssertionError, match='outside the bound'):
            td.assert_inside_bound(got, ref, names, mutant)


@pytest.mark.parametrize('d', sorted(HEADS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_mutant_exp_rounded_fails_the_bound_on_one_step_sums(dt, d):
    """An exponential rounded to the pipeline dtype before the sum is a second rounding: up to 1.5 ulps on a ``spread`` probability.
    One-step f32 sums (the walk windows; every step of an f32-sum run) show it outright.  Over several steps the worst case has to
    recur on the same element: with pipeline-dtype sums of three steps this mutant stays inside the bound, and the files say so."""
    got, ref, names = _mutant(dt, d, 'exp_rounded', 1, 'float32')
    worst = td.worst_by_kind(got, ref, names)
    print(f'exp_rounded {dt} d {d}: {td.report(worst)}')
    assert worst['spread'][0] > 1.2, worst
    with pytest.raises(AssertionError, match='outside the bound'):
        td.assert_inside_bound(got, ref, names, 'exp_rounded')
