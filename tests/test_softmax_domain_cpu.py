"""The inputs of ``tests/test_gpu_softmax_domain.py`` hold what that file relies on (no GPU): every step and head has its share of
plain, over and under rows, the oracle is finite on them, and the extreme rows do not depend on the summation order of q.k."""
import numpy as np
import pytest

import _softmax_domain as sd
from oracle import heatmap_oracle as ho

# (head_dim, heads): the routes of tests/test_gpu_layouts.py::ROUTES
SHAPES = [(64, 2), (40, 8), (80, 4), (160, 2)]
DTYPES = {'f16': np.float16, 'bf16': ho.BF16, 'f32': np.float32}
SHARE = 0.10
N_STEPS = 3


def _case(d, heads, hw, dt):
    np_dt = DTYPES[dt]
    steps, names = sd.build(hw, heads, d, np_dt, N_STEPS)
    return np_dt, steps, names, d ** -0.5


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('hw', sd.HWS)
@pytest.mark.parametrize('d,heads', SHAPES)
def test_every_step_and_head_has_its_share_of_every_class(d, heads, hw, dt):
    np_dt, steps, names, scale = _case(d, heads, hw, dt)
    for upcast in (False, True):
        cls = sd.row_classes(steps, heads, scale, np_dt, upcast=upcast)              # [steps, kept heads, hw]
        for c, name in enumerate(sd.CLASS_NAMES):
            share = (cls == c).mean(-1)
            assert share.min() >= SHARE, f'{name} (upcast {upcast}): {share.min():.3f} of the rows of some step and head'
        # what the slots are named for
        assert (cls[:, :, names == 'under'] == sd.UNDER).all()
        for name in ('tie2', 'tie3', 'last', 'over_all', 't0_high'):
            assert (names == name).sum() >= 8
            assert (cls[:, :, names == name] == sd.OVER).all(), name
        assert (cls[:, :, names == 't0_low'] == sd.PLAIN).all()
        assert ((cls[:, :, names == 'over'] == sd.OVER).mean(-1) >= 0.7).all()        # one level in four sits below the switch


@pytest.mark.parametrize('hw', sd.HWS)
def test_token_0_flavour_shares(hw):
    """``tap_mfma_kernel`` subtracts token 0's logit first: ``over`` is judged with the shifted sum, which cannot underflow (token
    0's own term is 1), so t0_low / t0_high stand where ``under`` does for the other flavours."""
    np_dt, steps, names, scale = _case(64, 2, hw, 'f16')
    cls = sd.row_classes(steps, 2, scale, np_dt, shifted=True)
    assert (cls != sd.UNDER).all()
    for c in (sd.PLAIN, sd.OVER):
        assert (cls == c).mean(-1).min() >= SHARE
    assert (names == 't0_low').sum() >= 8 and (names == 't0_high').sum() >= 8
    assert (cls[:, :, names == 't0_low'] == sd.OVER).all()                           # every other token 100 above token 0: redone
    assert (cls[:, :, names == 't0_high'] == sd.PLAIN).all()                         # every other token 100 below: the sum is 1
    assert (cls[:, :, names == 'under'] == sd.PLAIN).all() and (cls[:, :, names == 'over_all'] == sd.PLAIN).all()


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('hw', sd.HWS)
@pytest.mark.parametrize('d,heads', SHAPES)
def test_oracle_is_finite_and_extreme_rows_ignore_the_summation_order(d, heads, hw, dt):
    np_dt, steps, names, scale = _case(d, heads, hw, dt)
    extreme = names != 'plain'
    for q, k in steps:
        qh, kh = sd.to_bh(q, heads), sd.to_bh(k, heads)
        qr, kr = np.ascontiguousarray(qh[..., ::-1]), np.ascontiguousarray(kh[..., ::-1])      # the head_dim axis reversed
        for upcast in (False, True):
            probs = ho.attention_probs(qh, kh, scale, np_dt, upcast_attention=upcast)
            assert np.isfinite(np.asarray(probs, np.float32)).all()
            x, xr = sd.rounded_logits(qh, kh, scale, np_dt, upcast), sd.rounded_logits(qr, kr, scale, np_dt, upcast)
            np.testing.assert_array_equal(x[:, extreme], xr[:, extreme])
            if upcast:                                                               # ... which is no property of every row: the f32
                assert (x[:, ~extreme] != xr[:, ~extreme]).any()                     # logits of the plain rows do move with the order
            np.testing.assert_array_equal(np.asarray(ho.attention_probs(qr, kr, scale, np_dt, upcast_attention=upcast))[:, extreme],
                                          np.asarray(probs)[:, extreme])
            # ... and they are the float64 softmax of those logits, rounded once (see _check_against_softmax64)
            _check_against_softmax64(np.asarray(probs, np.float32), x, names, np_dt, dt)


def _check_against_softmax64(probs, x, names, np_dt, dt):
    """The oracle's softmax runs in f32 (as torch's does): its probabilities are the float64 ones to ~2^-22 relative BEFORE the rounding
    to the pipeline dtype, so where a float64 probability lies that close to a rounding boundary the two round apart (measured: 33
    of 543312 fp16 elements at head_dim 40, hw 576, all on rows whose 77 tokens all carry probability).  Hence: bit-equal on the
    fp16 and bf16 rows whose probability sits on one, two or three tokens (1, 1/2, 1/3 and exact zeros: nowhere near a boundary); within one
    ulp of the pipeline dtype everywhere, on at most 0.1 % of the elements; f32 pipelines within 2^-15 relative (an f32
    exp of an argument near -200 carries the rounding of that argument's product with log2 e: |x| 2^-23)."""
    want = np.asarray(sd.softmax64(x, np_dt), np.float32)
    diff = np.abs(probs.astype(np.float64) - want.astype(np.float64))
    if dt == 'f32':
        assert (diff <= 2.0 ** -15 * want + 1e-37).all()
        return
    ulp_rel, tiny = (2.0 ** -10, 2.0 ** -24) if dt == 'f16' else (2.0 ** -7, 2.0 ** -133)
    assert (diff <= ulp_rel * want + tiny).all()
    assert (diff[:, names != 'plain'] > 0).mean() <= 1e-3
    few = np.isin(names, ('over', 'tie2', 'tie3', 'last', 't0_high'))
    np.testing.assert_array_equal(probs[:, few], want[:, few])


def test_gain_hits_the_levels():
    """Exactly 48 / 96 / 192 at head_dim 64, within 6 % of the level at the other head dims."""
    for level, g in ((48, 2.0), (96, 4.0), (192, 8.0)):
        assert sd.gain(level, 64) == g
    for d in (40, 80, 160):
        for level in sd.OVER_LEVELS + sd.UNDER_LEVELS + (sd.T0_LEVEL,):
            assert abs(sd.gain(level, d) * sd.GAMMA * d ** 0.5 / level - 1.0) <= 0.06


# ---- daam_attend outputs: what a correct f32 softmax other than the oracle's can promise per class --------------------------------
ATTEND_CASES = [(dt, d, heads, hw) for dt in ('f16', 'bf16') for d, heads in ((64, 2), (80, 4)) for hw in sd.HWS]


@pytest.mark.parametrize('dt,d,heads,hw', ATTEND_CASES)
def test_emulated_fast_softmax_meets_the_attend_checks(dt, d, heads, hw):
    """``tests/test_gpu_softmax_domain.py::test_attend_by_row_class`` on ``sd.emulate_fast_probs`` in place of the kernel: the bound
    it sets per class -- every output within its own ulp plus one ulp on each probability of its row -- and the shares it asks
    (of the call; of the plain and over rows) hold for an f32 softmax that rounds its exponent once, so they ask nothing of the kernel
    that the number formats do not give.  The largest ``err / (ulp + slack)`` over all cases is 0.8826 (fp16, head_dim 80, hw 576,
    step 1, ``under``); the kernel measured 0.8826 there."""
    np_dt, scale, share = DTYPES[dt], d ** -0.5, 0.995 if dt == 'f16' else 0.99
    steps, _ = sd.build(hw, heads, d, np_dt, 2)
    for (q, k), v in zip(steps, sd.attend_values(hw, heads, d, np_dt, 2)):
        qh, kh, vh = (sd.to_bh(np.asarray(x, np.float32), heads) for x in (q, k, v))
        x = sd.rounded_logits(qh, kh, scale, np_dt)
        probs = np.asarray(ho.attention_probs(qh, kh, scale, np_dt), np.float64)
        mine = np.asarray(sd.emulate_fast_probs(x, np_dt), np.float64)
        assert (np.abs(mine - probs) <= sd.ulp_of(probs, np_dt)).all()                # a probability is at most one ulp off
        want = np.asarray(ho.attention_output(qh, kh, vh, scale, np_dt), np.float64)
        err = np.abs(np.asarray(sd.emulate_output(mine, vh, np_dt), np.float64) - want)
        ulp, slack, classes = sd.ulp_of(want, np_dt), sd.output_slack(probs, vh, np_dt), sd.classify(x)
        assert (err <= ulp + slack).all(), (err / (ulp + slack)).max()
        assert (err <= ulp).mean() >= share
        for c in (sd.PLAIN, sd.OVER):
            assert (err <= ulp)[classes == c].mean() >= share


def test_emulated_fast_softmax_misses_the_share_on_under_rows():
    """Why the share within one ulp is not asked of the ``under`` class: fp16, head_dim 80, hw 576, step 1.  44 of 354816 emulated
    probabilities round the other way than the oracle's; one of them, 0.316 at token 21, sits on the ``under`` rows of one level in
    one head, which all have the same Q row: 34 pixels, 16 of whose 80 outputs each are small enough by cancellation for one ulp of
    that probability to exceed their own ulp.  Share 0.99167 where the call keeps 0.9985; the kernel measured 0.99167 as well."""
    d, heads, hw, scale = 80, 4, 576, 80 ** -0.5
    (q, k), v = sd.build(hw, heads, d, np.float16, 2)[0][1], sd.attend_values(hw, heads, d, np.float16, 2)[1]
    qh, kh, vh = (sd.to_bh(np.asarray(x, np.float32), heads) for x in (q, k, v))
    x = sd.rounded_logits(qh, kh, scale, np.float16)
    mine = sd.emulate_fast_probs(x, np.float16)
    want = np.asarray(ho.attention_output(qh, kh, vh, scale, np.float16), np.float64)
    err = np.abs(np.asarray(sd.emulate_output(mine, vh, np.float16), np.float64) - want)
    within, under = err <= sd.ulp_of(want, np.float16), sd.classify(x) == sd.UNDER
    assert within[under].mean() < 0.995 <= within.mean()
    assert (~within[under]).sum() == 34 * 16 and (~within[under]).any(-1).sum() == 34
    worst = (err / (sd.ulp_of(want, np.float16) + sd.output_slack(ho.attention_probs(qh, kh, scale, np.float16), vh, np.float16)))[under].max()
    assert 0.5 < worst <= 1.0
