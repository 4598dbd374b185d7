"""The word-map epilogue on the device against the float64 oracle of ``tests/_epilogue_domain.py`` (which derives every bound;
``tests/test_epilogue_domain_cpu.py`` holds the oracle, the bounds and the cases to what this file relies on):

  1. ``normalize_``        n_rows 1 / 2 / 3 / 9 / 77, planes of 1 / 63 / 256 / 257 / 4096 pixels, square and rectangular entry points,
                           in place, the rows past ``n_rows`` untouched
  2. ``word_heat_map``     one index, a few, all content tokens, repeats, descending, 77 and 80 (``kMaxTokens``) indices
  3. ``expand_word_map``   every size set x plane kind x {min-max, absolute} x {values, threshold}: values inside the resize / min-max
                           bound, masks exact outside the ambiguous set, [0, 1] always; the peak planes' extremes; a value equal to
                           the threshold; a NaN and an inf source pixel
  4. ``word_masks``        the same planes through the batched kernels: bit-identical to the single-word calls, masks by the oracle
  5. ``mask_overlap``      the resize leg by the interval rule, one same-size soft pair

Every test prints its worst ``err / bound`` per plane kind, the ambiguous pixels and how many of them differ from the oracle, and how
many elements are not the bits of the f32 numpy restatement (information, not an assertion).  Run with ``-m gpu`` on an MI355X."""
import functools

import numpy as np
import pytest
import torch

import _epilogue_domain as ed
import test_gpu_word_masks as twm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
SENTINEL = -7.0


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(DEV)


def _bits_differ(got, emulated):
    return int((np.asarray(got, F32).view(np.int32) != np.asarray(emulated, F32).view(np.int32)).sum())


# ---- 1. normalize_ -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ed.NORMALIZE_KINDS)
def test_normalize(kind):
    from daam_amd.engine import HeatMapEngine
    engines = {True: HeatMapEngine(1, out_side=16), False: HeatMapEngine(1, out_hw=(7, 9))}
    worst, off_bits, cases = 0.0, 0, 0
    try:
        for rows in ed.NORMALIZE_ROWS:
            for h, w in ed.NORMALIZE_PLANES:
                maps = ed.planes(kind, rows, h, w)
                ref = ed.normalize(maps)
                buf = torch.full((rows + 2, h, w), SENTINEL, device=DEV)
                buf[:rows] = _dev(maps)
                eng = engines[h == w]
                eng._require_device(buf)
                out = eng.normalize_(buf[:rows])
                assert out.data_ptr() == buf.data_ptr()                                        # in place
                got = buf.cpu().numpy()
                assert (got[rows:] == SENTINEL).all(), (rows, h, w)                            # n_rows bounds the writes
                keep = ~ref['free']
                assert np.isfinite(got[:rows][keep]).all(), (rows, h, w)
                r = ed.ratio(got[:rows], ref, skip=ref['free'])
                assert r <= 1.0, f'{kind} rows {rows} plane {h}x{w}: err / bound {r:.3f}'
                worst = max(worst, r)
                off_bits += _bits_differ(got[:rows], ed.emulate_normalize(maps))
                cases += 1
    finally:
        for eng in engines.values():
            eng.close()
    print(f'normalize {kind}: {cases} cases, worst err / bound {worst:.3f}, {off_bits} elements not the bits of the f32 restatement')


# ---- 2. word_heat_map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ed.WORD_KINDS)
def test_word_heat_map(kind):
    from daam_amd import engine as E
    worst, off_bits = 0.0, 0
    for h, w in ((16, 24), (32, 32)):
        maps = ed.planes(kind, 77, h, w)
        gm = _dev(maps)
        for name, idxs in ed.WORD_LISTS.items():
            got = E.word_heat_map(gm, idxs).cpu().numpy()
            r = ed.ratio(got, ed.word_mean(maps, idxs))
            assert np.isfinite(got).all() and r <= 1.0, f'{kind} {h}x{w} {name}: err / bound {r:.3f}'
            worst = max(worst, r)
            off_bits += _bits_differ(got, ed.emulate_word_mean(maps, idxs))
    print(f'word mean {kind}: worst err / bound {worst:.3f}, {off_bits} elements not the bits of the f32 restatement')


# ---- 3. expand_word_map ----------------------------------------------------------------------------------------------------------------------
def _peak_checks(E, word, kind, sizes, got_minmax):
    """The normalised extremes from the kernel's own ``absolute`` values: the minimum pixel is exactly 0, the maximum within 2 ulp of
    ``range / (range + 1e-8)``; the peak is the last (first) pixel."""
    (_, _), (oh, ow) = sizes
    v = E.expand_word_map(word, oh, ow, absolute=True).cpu().numpy().reshape(-1)
    q = got_minmax.reshape(-1)
    lo, hi = v.min(), v.max()
    top = (hi - lo) / ((hi - lo) + ed.EPS_RANGE)
    at_lo, at_hi = int(v.argmin()), int(v.argmax())
    assert (at_hi == v.size - 1) if kind == 'peak_last' else (at_lo == 0), (kind, sizes, at_lo, at_hi)
    assert q[at_lo] == 0.0 and q.min() == 0.0, (kind, sizes, q[at_lo])
    assert abs(float(q[at_hi]) - float(top)) <= 2 * ed.ulp(top) and q.max() == q[at_hi], (kind, sizes, q[at_hi], top)


@pytest.mark.parametrize('sizes', ed.SIZE_SETS, ids=lambda s: f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}')
def test_expand_word_map(sizes):
    from daam_amd import engine as E
    (h, w), (oh, ow) = sizes
    worst, ambiguous, flipped, off_bits, cases = {}, 0, 0, 0, 0
    extra = [(k, a, t) for s, k, a, t in ed.expand_cases() if s == sizes and (a, t) not in ed.MODES]
    for kind in ed.EXPAND_KINDS:
        plane = ed.word_plane(kind, h, w)
        word = _dev(plane)
        res, emulated = ed.resize(plane, oh, ow), ed.emulate_resize(plane, oh, ow)
        for absolute, threshold in list(ed.MODES) + [(a, t) for k, a, t in extra if k == kind]:
            what = f'{sizes} {kind} absolute={absolute} threshold={threshold}'
            got = E.expand_word_map(word, oh, ow, absolute=absolute, threshold=threshold).cpu().numpy()
            ref = ed.expand(plane, oh, ow, absolute, threshold, res=res)
            figures = ed.check_expand(got, ref, what)
            if not absolute:
                raw = got if threshold is None else E.expand_word_map(word, oh, ow).cpu().numpy()
                assert raw.min() >= 0.0 and raw.max() <= 1.0, what                             # the range rule, always
                if (oh, ow) == (1, 1):
                    assert raw[0, 0] == 0.0, what
            if 'ratio' in figures:
                worst[kind] = max(worst.get(kind, 0.0), figures['ratio'])
            elif not figures['ill']:
                assert figures['ambiguous'] <= ed.AMBIGUOUS_CAP * got.size, what
                ambiguous, flipped = ambiguous + figures['ambiguous'], flipped + figures['flipped']
            off_bits += _bits_differ(got, ed.emulate_expand(plane, oh, ow, absolute, threshold, resized=emulated))
            cases += 1
            if kind in ('peak_last', 'peak_first') and not absolute and threshold is None and not ed.may_be_ill(sizes, kind):
                _peak_checks(E, word, kind, sizes, got)
    print(f'expand {sizes}: {cases} cases, worst err / bound -- ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items())
          + f'; {ambiguous} ambiguous pixels, {flipped} of them differ; {off_bits} elements not the bits of the f32 restatement')


def test_a_value_equal_to_the_threshold_is_not_above_it():
    """``absolute`` at identity sizes is a copy: an eighth of the pixels equal 0.5 and must give 0 (``>``, not ``>=``) -- through the
    single-word kernel and through ``word_masks``."""
    from daam_amd import engine as E
    plane = ed.dyadic_plane(12, 20)
    ref = ed.expand(plane, 12, 20, True, 0.5)
    assert not ref['ambiguous'].any() and (plane == F32(0.5)).sum() >= 12
    got = E.expand_word_map(_dev(plane), 12, 20, absolute=True, threshold=0.5).cpu().numpy()
    assert np.array_equal(got, ref['want'])
    _, masks, _ = E.word_masks(_dev(plane[None]), [[0]], 12, 20, absolute=True, threshold=0.5)
    assert np.array_equal(masks[0].cpu().numpy(), ref['want'].astype(np.uint8))


def test_nan_and_inf_source_pixels():
    """What comes back for a NaN / an inf source pixel, next to torch's CPU semantics restated in numpy (``interpolate`` propagates
    them through every product, ``min`` / ``max`` propagate a NaN).  The resize agrees: the same pixels are NaN / +-inf.  The min-max
    step differs, and DESIGN section 4 says so: the kernel's ``fminf`` / ``fmaxf`` skip a NaN, so the pixels outside the NaN's window
    are normalised by the extremes of the others (asserted: inside the min-max bound of the oracle with NaN-skipping extremes) where
    the reference returns NaN everywhere.  With an inf pixel both return NaN or +-inf everywhere that matters (recorded)."""
    from daam_amd import engine as E
    sizes = ((16, 24), (37, 53))
    (h, w), (oh, ow) = sizes
    for bad in (np.nan, np.inf):
        plane = ed.word_plane('signed', h, w).copy()
        plane[5, 7] = bad
        with np.errstate(invalid='ignore', over='ignore'):
            emulated = ed.emulate_resize(plane, oh, ow)
            got = E.expand_word_map(_dev(plane), oh, ow, absolute=True).cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(emulated))
            assert np.array_equal(np.isposinf(got), np.isposinf(emulated)) and np.array_equal(np.isneginf(got), np.isneginf(emulated))
            fine = np.isfinite(emulated)
            res = ed.resize(plane, oh, ow)
            err = np.abs(got.astype(np.float64) - res['want'])
            assert (err[fine] <= res['bound'][fine]).all()
            q = E.expand_word_map(_dev(plane), oh, ow).cpu().numpy()
            reference = (emulated - emulated.min()) / (emulated.max() - emulated.min() + ed.EPS_RANGE)      # numpy min / max propagate NaN
            print(f'source pixel {bad}: absolute -- {int(np.isnan(got).sum())} NaN, {int(np.isinf(got).sum())} inf of {got.size}; min-max -- '
                  f'kernel {int(np.isnan(q).sum())} NaN, {int(np.isinf(q).sum())} inf, reference {int(np.isnan(reference).sum())} NaN')
            if np.isnan(bad):
                assert np.isnan(reference).all()
                assert np.array_equal(np.isnan(q), np.isnan(got))
                ref = ed.minmax(res, 'ignore nan')
                assert not ref['ill']
                err = np.abs(q.astype(np.float64) - ref['want'])
                assert (err[fine] <= ref['bound'][fine]).all()
                assert q[fine].min() == 0.0 and q[fine].max() <= 1.0


# ---- 4. word_masks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_words', [1, 3, 32])
@pytest.mark.parametrize('sizes', ed.MASK_SIZES, ids=lambda s: f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}')
def test_word_masks(sizes, n_words):
    """Bit-identical to the single-word calls (``test_gpu_word_masks._check``: word maps, masks, labels, ties to the lower index), and the
    masks of the first words and the last against the float64 oracle of the word map the device returned."""
    from daam_amd import engine as E
    (h, w), out = sizes
    words = twm._words(n_words)
    ambiguous = flipped = 0
    for kind in ed.MASK_KINDS:
        maps = ed.planes(kind, twm.ROWS, h, w)
        maps[14:] = 0                                      # the all-zero word of ``_words``
        gm = _dev(maps)
        for absolute in (False, True):
            masks, _ = twm._check(gm, words, out, absolute, 0.4)
            word_maps = E.word_masks(gm, words, *out, absolute=absolute, threshold=0.4, labels=False)[0].cpu().numpy()
            for j in sorted({0, 1, 2, n_words - 1} & set(range(n_words))):
                ref = ed.expand(word_maps[j], *out, absolute, 0.4)
                assert not ref['ill'], (sizes, kind, j)
                amb, flip, wrong = ed.mask_mismatches(masks[j].cpu().numpy(), ref)
                assert wrong == 0 and amb <= ed.AMBIGUOUS_CAP * ref['want'].size, (sizes, kind, absolute, j, amb, wrong)
                ambiguous, flipped = ambiguous + amb, flipped + flip
        # the same index list twice: every pixel a tie, the label is the first word's
        _, masks, labels = E.word_masks(gm, [[2, 3], [2, 3]], *out, threshold=0.4)
        assert torch.equal(masks[0], masks[1]) and not bool((labels == 1).any())
        assert torch.equal(labels == 0, masks[0] != 0) and bool(((labels == 0) | (labels == 255)).all())
    print(f'word_masks {sizes} W={n_words}: {ambiguous} ambiguous pixels, {flipped} of them differ')


# ---- 5. mask_overlap -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _overlap_ref(kind, shape, seed):
    return ed.overlap(ed.overlap_prediction(kind, *shape[0], seed=seed), ed.truth(*shape[1], seed=seed))


@pytest.mark.parametrize('shape', ed.OVERLAP_SHAPES, ids=lambda s: f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}')
def test_mask_overlap_with_resize(shape):
    from daam_amd.evaluate import mask_overlap
    (ah, aw), (bh, bw) = shape
    ambiguous = inside = 0
    for kind in ed.OVERLAP_KINDS:
        for n_pairs in (1, 3):
            a = np.stack([ed.overlap_prediction(kind, ah, aw, seed=i) for i in range(n_pairs)])
            b = np.stack([ed.truth(bh, bw, seed=i) for i in range(n_pairs)])
            got = mask_overlap(_dev(a), _dev(b)).cpu().numpy().astype(np.float64)
            for i in range(n_pairs):
                ref = _overlap_ref(kind, shape, i)
                assert ref['ambiguous'].sum() <= ed.AMBIGUOUS_CAP * bh * bw
                assert (ref['lo'] <= got[i]).all() and (got[i] <= ref['hi']).all(), (shape, kind, n_pairs, i, got[i], ref['lo'], ref['hi'])
                assert got[i][2] == ref['lo'][2]
                ambiguous += int(ref['ambiguous'].sum())
                inside += int(got[i][1] - ref['lo'][1])
    print(f'mask_overlap {shape}: {ambiguous} ambiguous pixels, {inside} of them counted as set')


def test_mask_overlap_same_size_soft():
    from daam_amd.evaluate import mask_overlap
    a = np.stack([ed.overlap_prediction('soft', 64, 64, seed=i) for i in range(3)])
    b = np.stack([ed.overlap_prediction('soft', 64, 64, seed=10 + i) for i in range(3)])
    got = mask_overlap(_dev(a), _dev(b)).cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(3):
        ref = ed.overlap_same_size(a[i], b[i])
        worst = max(worst, float((np.abs(got[i] - ref['want']) / ref['bound']).max()))
    print(f'mask_overlap same size, soft: worst err / bound {worst:.3f}')
    assert worst <= 1.0
