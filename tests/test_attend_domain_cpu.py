"""The inputs and the bound of ``tests/test_gpu_attend_domain.py`` hold what that file relies on (no GPU): the logits do not depend on
the summation order, every pixel count has every row kind, the gap rows' minor probabilities are what their names say in fp16, a
kernel that dropped the fp16-subnormal probabilities would be caught, and a correct f32 implementation other than the oracle's stays
inside the bound."""
import numpy as np
import pytest

import _attend_domain as ad
import _softmax_domain as sd
from oracle import heatmap_oracle as ho

DTYPES = {'f16': np.float16, 'bf16': ho.BF16}
# every pixel count tests/test_gpu_attend_domain.py runs
GPU_HWS = (8, 24, 40, 72, 120, 136, 208, 256, 264)
# (head_dim, heads, hw) of its V-set cases
VSET_SHAPES = [(64, 2, 256), (64, 2, 136), (80, 4, 256), (80, 4, 136)]
SUBNORMAL_MIN, NORMAL_MIN = 2.0 ** -24, 2.0 ** -14


def _minor(probs, names, kind, step):
    """The probabilities of the tokens that are not the designed one, on the rows of ``kind``: [BH, rows, 76]."""
    rows = np.nonzero(names == kind)[0]
    out = []
    for p in rows:
        keep = np.arange(ad.TOKENS) != ad.designed_token(p, step)
        out.append(probs[:, p][:, keep])
    return np.stack(out, 1)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('d', ad.HEAD_DIMS)
def test_no_logit_depends_on_the_summation_order(d, dt):
    """Reversing the head_dim axis of Q and K changes no rounded logit and no probability, on any row."""
    np_dt, scale = DTYPES[dt], d ** -0.5
    steps, _ = ad.build(40, 3, d, np_dt, 2)
    for q, k in steps:
        assert np.abs(np.asarray(q, np.float32)).max() <= 3.0 and np.abs(np.asarray(k, np.float32)).max() <= 3.0
        assert np.array_equal(np.asarray(q, np.float32) * 4 % 1, np.zeros(q.shape)) and np.array_equal(np.asarray(k, np.float32) * 4 % 1, np.zeros(k.shape))
        qh, kh = sd.to_bh(np.asarray(q, np.float32), 3), sd.to_bh(np.asarray(k, np.float32), 3)
        qr, kr = np.ascontiguousarray(qh[..., ::-1]), np.ascontiguousarray(kh[..., ::-1])
        np.testing.assert_array_equal(sd.rounded_logits(qh, kh, scale, np_dt), sd.rounded_logits(qr, kr, scale, np_dt))
        np.testing.assert_array_equal(np.asarray(ho.attention_probs(qh, kh, scale, np_dt)), np.asarray(ho.attention_probs(qr, kr, scale, np_dt)))


@pytest.mark.parametrize('hw', GPU_HWS)
def test_every_pixel_count_has_every_kind(hw):
    names = ad.kind_names(hw)
    for kind in ad.KIND_NAMES:
        assert (names == kind).any(), (hw, kind)
    # ... and every lane of a 16-pixel column group meets every kind once the layer has 13 groups
    big = ad.kind_names(16 * 13)
    for lane in range(16):
        assert set(big[lane::16]) == set(ad.KIND_NAMES)


@pytest.mark.parametrize('d', ad.HEAD_DIMS)
def test_gap_rows_are_what_their_names_say_in_fp16(d):
    """gap8: every minor probability is an fp16 normal; gap12 and gap16: a non-zero fp16 subnormal (gap16: at most 32 ulps); gap20: zero.
    The designed token keeps more than 0.8 of a gap8 row and 0.998 of the others; a tie2 row has two tokens within one ulp of each other above 0.48."""
    scale = d ** -0.5
    steps, names = ad.build(136, 3, d, np.float16, 2)
    for s, (q, k) in enumerate(steps):
        probs = np.asarray(ho.attention_probs(sd.to_bh(q, 3), sd.to_bh(k, 3), scale, np.float16), np.float64)
        m8, m12, m16, m20 = (_minor(probs, names, kind, s) for kind in ('gap8', 'gap12', 'gap16', 'gap20'))
        assert (m8 >= NORMAL_MIN).all() and m8.max() < 2.0 ** -7
        assert (m12 >= SUBNORMAL_MIN).all() and (m12 < NORMAL_MIN).all()
        assert (m16 >= SUBNORMAL_MIN).all() and (m16 <= 32 * SUBNORMAL_MIN).all()
        assert (m20 == 0).all()
        for kind in ad.GAPS:
            rows = np.nonzero(names == kind)[0]
            lead = np.array([probs[:, p, ad.designed_token(p, s)] for p in rows])
            assert (lead > (0.8 if kind == 'gap8' else 0.998)).all(), (kind, lead.min())
        for p in np.nonzero(names == 'tie2')[0]:
            top = np.sort(probs[:, p], -1)[:, -2:]
            assert (top > 0.48).all() and (np.abs(top[:, 0] - top[:, 1]) <= 2.0 ** -11).all()
        # the rotation reaches every designed token on every gap kind
        for kind in ad.GAPS:
            assert {ad.designed_token(p, s) for p in np.nonzero(names == kind)[0]} == set(ad.DESIGNED)


def test_value_sets_have_their_levels():
    for np_dt in DTYPES.values():
        for v_set in ad.V_SETS:
            for s, v in enumerate(ad.values(v_set, 2, 64, np_dt, 3)):
                v = np.abs(np.asarray(v, np.float64))
                level, _ = ad.levels(v_set, s)
                assert ((v >= 2.0 ** level[None, :, None]) & (v <= 2.0 ** (level[None, :, None] + 1))).all()      # <=: a subnormal may round up
    tiny = np.abs(np.asarray(ad.values('tiny', 2, 64, np.float16, 1)[0], np.float64))
    assert ((tiny[:, 1::2] > 0) & (tiny[:, 1::2] < NORMAL_MIN)).all() and (tiny[:, ::2] >= 1).all()      # fp16 subnormal, none flushed
    heavy = np.abs(np.asarray(ad.values('heavy_minor', 2, 64, np.float16, 1)[0], np.float64))
    assert (heavy[:, list(ad.DESIGNED)] < 2).all() and (np.delete(heavy, ad.DESIGNED, 1) >= 2.0 ** ad.HEAVY).all()
    mixed = np.asarray(ad.values('mixed', 2, 64, np.float16, 1)[0], np.float64)
    assert (mixed[:, ::2] > 0).all() and (mixed[:, 1::2] < 0).all()


@pytest.mark.parametrize('d,heads,hw', VSET_SHAPES)
def test_dropped_subnormal_probabilities_are_visible(d, heads, hw):
    """The oracle's output with every fp16-subnormal probability set to zero (an MFMA operand flushed, a slot skipped) on the
    ``heavy_minor`` values: at least 10 x the bound on the gap12 rows, or the inputs do not test what they claim.  (gap16 rows carry one
    to eight ulps per token: dropping them stays inside what one ulp on every probability allows, and the bound says so.)"""
    scale = d ** -0.5
    steps, names = ad.build(hw, heads, d, np.float16, 2)
    for (q, k), v in zip(steps, ad.values('heavy_minor', heads, d, np.float16, 2)):
        ref = ad.reference(q, k, v, heads, scale, np.float16)
        flushed = np.where(ref['probs'] < NORMAL_MIN, 0.0, ref['probs'])
        worst = ad.worst_by_kind(sd.emulate_output(flushed, ref['vh'], np.float16), ref, names)
        print(f'subnormal probabilities dropped, d {d} hw {hw}: worst err / bound -- {ad.report(worst)}')
        assert worst['gap12'][0] >= 10.0, worst['gap12']
        for kind in ('gap8', 'gap20'):                            # nothing to drop there: normal, resp. zero already
            assert worst[kind][0] <= 1.0, (kind, worst[kind])


def _emulated_worst(dt, v_set, d, heads, hw, n_steps=2):
    np_dt, scale = DTYPES[dt], d ** -0.5
    steps, names = ad.build(hw, heads, d, np_dt, n_steps)
    total = {}
    for (q, k), v in zip(steps, ad.values(v_set, heads, d, np_dt, n_steps)):
        ref = ad.reference(q, k, v, heads, scale, np_dt)
        mine = np.asarray(sd.emulate_fast_probs(sd.rounded_logits(ref['qh'], ref['kh'], scale, np_dt), np_dt), np.float64)
        assert (np.abs(mine - ref['probs']) <= sd.ulp_of(ref['probs'], np_dt)).all()             # a probability is at most one ulp off
        for kind, (r, at) in ad.worst_by_kind(sd.emulate_output(mine, ref['vh'], np_dt), ref, names).items():
            total[kind] = max(total.get(kind, 0.0), r)
    return total


@pytest.mark.parametrize('v_set', ad.V_SETS)
@pytest.mark.parametrize('dt', list(DTYPES))
def test_the_bound_fits_an_emulated_correct_kernel(dt, v_set):
    """``sd.emulate_fast_probs`` (the kernels' fast softmax in numpy) followed by ``sd.emulate_output`` (f32 sum, one rounding) on
    every V-set case of the GPU file: inside the bound everywhere.  The bound is the issue's derivation unchanged -- the emulation
    needed no wider accumulation term."""
    worst = {}
    for d, heads, hw in VSET_SHAPES:
        for kind, r in _emulated_worst(dt, v_set, d, heads, hw).items():
            worst[kind] = max(worst.get(kind, 0.0), r)
    print(f'emulated kernel, {dt} {v_set}: worst err / bound per kind -- ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('dt', list(DTYPES))
def test_the_bound_fits_an_emulated_correct_kernel_at_every_head_dim(dt):
    worst = {d: max(_emulated_worst(dt, 'mixed', d, 3, 136, 1).values()) for d in ad.HEAD_DIMS}
    print(f'emulated kernel, {dt} mixed, worst err / bound per head dim -- ' + ', '.join(f'{d}: {r:.3f}' for d, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst
