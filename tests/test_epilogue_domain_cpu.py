"""The planes, the oracle and the bounds of ``tests/test_gpu_epilogue_domain.py`` hold what that file relies on (no GPU): the f32
coefficients are the float64 ones up to their Horner roundings; an f32 numpy emulation of every kernel, in its operation order, stays
inside every bound on every case of the GPU file; every listed mutant of that emulation misses a bound on a listed case; few pixels
are ambiguous and only the listed min-max cases are ill-conditioned."""
import functools

import numpy as np
import pytest

import _epilogue_domain as ed

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _plane(kind, h, w):
    return ed.word_plane(kind, h, w)


@functools.lru_cache(maxsize=None)
def _resized(kind, sizes):
    (h, w), (oh, ow) = sizes
    return ed.resize(_plane(kind, h, w), oh, ow), ed.emulate_resize(_plane(kind, h, w), oh, ow)


def _expand_pair(sizes, kind, absolute, threshold, **mutant):
    (h, w), (oh, ow) = sizes
    plane = _plane(kind, h, w)
    res, emulated = _resized(kind, sizes)
    if any(k in mutant for k in ('swap', 'clamp_short', 'a')):
        emulated = None
    return (ed.emulate_expand(plane, oh, ow, absolute, threshold, resized=emulated, **mutant),
            ed.expand(plane, oh, ow, absolute, threshold, res=res))


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------
def _axes():
    return sorted({(src[a], out[a]) for src, out in ed.SIZE_SETS + ed.OVERLAP_SHAPES for a in (0, 1) if src != out})


def test_f32_coefficients_are_the_float64_ones_up_to_their_roundings():
    """At the same (f32) t: inside the running error bound of the Horner forms, itself at most 12 x 2^-24 x the largest intermediate
    (6: ``p x + 8 A`` at x = 2).  With float64 coordinates as well: the source coordinate is off by up to 3 u (|src| + 1) -- ``sc``,
    the product and the subtraction -- and a weight's slope is at most 1.35, which is why the GPU bound keeps the coefficients out."""
    worst, worst_dense = 0.0, 0.0
    for n_in, n_out in _axes():
        idx, w32 = ed.taps(n_in, n_out)
        _, t = ed.source_coords(n_in, n_out)
        w64 = ed.cubic_weights(t.astype(np.float64), np.float64)
        err, big = ed.horner_error(t)
        assert big.max() <= 6.0 and (err <= 12 * ed.U * 6.0).all()
        assert (np.abs(w32 - w64) <= err).all(), (n_in, n_out, (np.abs(w32 - w64) / err).max())
        worst = max(worst, float((np.abs(w32 - w64) / err).max()))
        assert (np.abs(w64.sum(1) - 1.0) <= 1e-15).all()
        i64, c64 = ed.coefficients64(n_in, n_out)
        src = n_in / n_out * (np.arange(n_out) + 0.5) - 0.5
        allowed = 4 * (1.35 * 3 * ed.U * (np.abs(src) + 1.0) + err.max())
        diff = np.abs(ed.dense(idx, w32, n_in) - ed.dense(i64, c64, n_in)).max(1)
        assert (diff <= allowed).all(), (n_in, n_out, (diff / allowed).max())
        worst_dense = max(worst_dense, float((diff / allowed).max()))
    print(f'f32 coefficients: worst err / bound {worst:.3f} at the same t, {worst_dense:.3f} against float64 coordinates')


# ---- the emulation stays inside -------------------------------------------------------------------------------------------------------
def test_emulated_normalize_stays_inside():
    worst = {}
    for kind in ed.NORMALIZE_KINDS:
        for rows in ed.NORMALIZE_ROWS:
            for h, w in ed.NORMALIZE_PLANES:
                maps = ed.planes(kind, rows, h, w)
                ref = ed.normalize(maps)
                free_pixels = int(ref['free'][0].sum())
                assert free_pixels <= (max(1, h * w // 1000) if kind == 'signed' else 0), (kind, rows, h, w, free_pixels)
                if kind != 'signed':                                        # the issue's form for non-negative planes
                    assert (ref['bound'] <= (rows + 2) * ed.U * np.abs(ref['want']) * (1 + 1e-4)).all()
                r = ed.ratio(ed.emulate_normalize(maps), ref, skip=ref['free'])
                worst[kind] = max(worst.get(kind, 0.0), r)
    print('emulated normalize, worst err / bound -- ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_emulated_word_mean_stays_inside():
    worst = {}
    for kind in ed.WORD_KINDS:
        maps = ed.planes(kind, 77, 16, 24)
        for name, idxs in ed.WORD_LISTS.items():
            worst[kind] = max(worst.get(kind, 0.0), ed.ratio(ed.emulate_word_mean(maps, idxs), ed.word_mean(maps, idxs)))
    print('emulated word mean, worst err / bound -- ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_emulated_expand_stays_inside_and_the_caps_hold():
    """Every expand case of the GPU file: values inside their bound, masks exact outside the ambiguous set, the range rule on the
    ill-conditioned planes; ambiguous pixels <= 2e-3 of every case; ill-conditioned only where listed."""
    worst, most, ill = {}, (0.0, ''), set()
    for sizes, kind, absolute, threshold in ed.expand_cases():
        what = f'{sizes} {kind} absolute={absolute} threshold={threshold}'
        got, ref = _expand_pair(sizes, kind, absolute, threshold)
        if ref['ill']:
            assert ed.may_be_ill(sizes, kind), f'{what}: ill-conditioned, and not listed'
            ill.add((sizes, kind))
        figures = ed.check_expand(got, ref, what)
        if 'ratio' in figures:
            worst[kind] = max(worst.get(kind, 0.0), figures['ratio'])
        elif not figures['ill']:
            share = figures['ambiguous'] / got.size
            assert share <= ed.AMBIGUOUS_CAP, f'{what}: {figures["ambiguous"]} of {got.size} pixels ambiguous'
            most = max(most, (share, what))
    print('emulated expand, worst err / bound -- ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items()))
    print(f'largest ambiguous share {most[0]:.2e} ({most[1]}); {len(ill)} ill-conditioned (sizes, kind) pairs')
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('kind', ('peak_last', 'peak_first'))
def test_the_peak_is_the_last_or_first_output_pixel(kind):
    """... alone, wherever the peak's source pixel reaches the output at all, so a lane dropped there moves every normalised value."""
    for sizes in ed.SIZE_SETS:
        (h, w), (oh, ow) = sizes
        if (h, w) == (1, 1) or (oh, ow) == (1, 1):
            continue
        want = ed.resize(_plane(kind, h, w), oh, ow)['want'].reshape(-1)
        if kind == 'peak_last':
            assert want.argmax() == want.size - 1 and want[-1] > 0.35 and np.sort(want)[-2] < want[-1] - 0.01, sizes
        else:
            assert want.argmin() == 0 and want[0] < 0.15 and np.sort(want)[1] > want[0] + 0.01, sizes


def test_emulated_overlap_stays_inside_and_few_pixels_are_ambiguous():
    most = (0.0, '')
    for (ah, aw), (bh, bw) in ed.OVERLAP_SHAPES:
        for kind in ed.OVERLAP_KINDS:
            a, b = ed.overlap_prediction(kind, ah, aw), ed.truth(bh, bw)
            ref = ed.overlap(a, b)
            got = ed.emulate_overlap(a, b)
            assert (ref['lo'] <= got).all() and (got <= ref['hi']).all(), ((ah, aw), (bh, bw), kind, got, ref['lo'], ref['hi'])
            share = ref['ambiguous'].mean()
            assert share <= ed.AMBIGUOUS_CAP, ((ah, aw), (bh, bw), kind, int(ref['ambiguous'].sum()))
            most = max(most, (float(share), f'{ah}x{aw} -> {bh}x{bw} {kind}'))
            if kind == 'blocks' and (ah, aw) != (1, 1):                 # both answers occur
                assert 0 < ref['lo'][1] < bh * bw
    print(f'overlap: largest ambiguous share {most[0]:.2e} ({most[1]})')
    a, b = ed.overlap_prediction('soft', 64, 64), ed.overlap_prediction('soft', 64, 64, seed=1)
    ref = ed.overlap_same_size(a, b)
    got = np.array([(a * b).sum(dtype=F32), a.sum(dtype=F32), b.sum(dtype=F32)], np.float64)
    assert (np.abs(got - ref['want']) <= ref['bound']).all()


# ---- every mutant misses a bound ----------------------------------------------------------------------------------------------------------
RECT = ((16, 24), (37, 53))
MUTANTS = [
    ('wx and wy swapped', RECT, 'signed', True, None, dict(swap=True)),
    ('a tap clamped to in - 2', RECT, 'signed', True, None, dict(clamp_short=True)),
    ('a tap clamped to in - 2, 2 x 2 source', ((2, 2), (9, 9)), 'levels', True, None, dict(clamp_short=True)),
    ('A = -0.5', ((64, 64), (200, 333)), 'real', True, None, dict(a=-0.5)),
    ('A = -0.5 at exact coefficients', ((64, 64), (128, 128)), 'levels', True, None, dict(a=-0.5)),
    ('min / max over whole waves only, peak in the tail', RECT, 'peak_last', False, None, dict(whole_waves_only=True)),
    ('min / max over whole waves only, fewer than 64 outputs', ((8, 8), (3, 3)), 'signed', False, None, dict(whole_waves_only=True)),
    ('signed-int compare of the bit patterns', RECT, 'negative', False, None, dict(int_order=True)),
    ('signed-int compare, minimum at the first pixel', ((24, 16), (16, 24)), 'peak_first', False, None, dict(int_order=True)),
    ('the 1e-8 dropped', ((48, 48), (32, 32)), 'tiny', False, None, dict(drop_eps=True)),
]


@pytest.mark.parametrize('name,sizes,kind,absolute,threshold,mutant', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_resize_and_minmax_mutants_miss_the_bound(name, sizes, kind, absolute, threshold, mutant):
    got, ref = _expand_pair(sizes, kind, absolute, threshold, **mutant)
    assert not ref['ill']
    with np.errstate(invalid='ignore'):
        r = ed.ratio(np.where(np.isfinite(got), got, np.inf), ref)
    print(f'{name} on {sizes} {kind}: err / bound {r:.3g}')
    assert r >= 10.0, r
    with pytest.raises(AssertionError):
        ed.check_expand(got, ref, name)


def test_ge_for_gt_is_caught_on_values_equal_to_the_threshold():
    """``absolute`` at identity sizes is a copy (bound 0): the eighth of ``dyadic_plane`` that equals 0.5 must give 0."""
    plane = ed.dyadic_plane(12, 20)
    ref = ed.expand(plane, 12, 20, True, 0.5)
    assert (plane == F32(0.5)).sum() >= 12 and not ref['ambiguous'].any()
    ed.check_expand(ed.emulate_expand(plane, 12, 20, True, 0.5), ref, 'correct')
    wrong = ed.mask_mismatches(ed.emulate_expand(plane, 12, 20, True, 0.5, ge=True), ref)[2]
    print(f'>= for >: {wrong} pixels differ')
    assert wrong == int((plane == F32(0.5)).sum())
    # ... and after a power-of-two upscale of a constant dyadic plane every value IS the threshold: all ambiguous, which is why the
    # identity case carries this mutant
    up = ed.expand(np.full((8, 8), 0.5, F32), 16, 16, True, 0.5)
    assert (up['value'] == 0.5).all() and up['ambiguous'].all()


def test_dropped_epsilon_and_distinct_mean_miss_the_bound():
    maps = ed.planes('zero_content', 9, 16, 16)
    ref = ed.normalize(maps)
    got = ed.emulate_normalize(maps, drop_eps=True)
    assert not np.isfinite(got).all()                                       # 0 / 0 where the content is all zero
    maps = ed.planes('tiny', 9, 16, 16)
    r = ed.ratio(ed.emulate_normalize(maps, drop_eps=True), ed.normalize(maps))
    print(f'the 1e-6 dropped on tiny: err / bound {r:.3g}')
    assert r >= 10.0
    for kind in ed.WORD_KINDS:
        maps = ed.planes(kind, 77, 16, 24)
        for name in ('repeats', '80 with repeats'):
            idxs = ed.WORD_LISTS[name]
            r = ed.ratio(ed.emulate_word_mean(maps, idxs, distinct=True), ed.word_mean(maps, idxs))
            print(f'mean over the distinct indices, {kind} {name}: err / bound {r:.3g}')
            assert r >= 10.0


def test_planes_are_what_their_names_say():
    for h, w in ((16, 24), (64, 64)):
        real = ed.planes('real', 9, h, w).astype(np.float64)
        assert (real[0] >= 50).all() and (real[-1] >= 1).all() and (real[-1] < 2).all()
        assert (real[1:-1] > 1e-5).all() and (real[1:-1] < 2e-2).all()
        signed = ed.planes('signed', 9, h, w)
        assert (signed < 0).any() and (signed > 0).any() and (np.signbit(signed) & (signed == 0)).sum() >= 8
        assert (ed.planes('negative', 9, h, w) < 0).all()
        lev = ed.planes('levels', 9, h, w)
        assert lev.min() >= 0 and lev[lev > 0].min() < 2.0 ** -18 and lev.max() > 4.0
        tiny = ed.word_plane('tiny', h, w).astype(np.float64)
        assert 0.1 <= (tiny.max() - tiny.min()) / float(ed.EPS_RANGE) <= 2.0
        assert 1e-3 <= ed.planes('tiny', 9, h, w)[1:-1].sum(0).max() / float(ed.EPS_NORM) <= 0.1
        zc = ed.planes('zero_content', 9, h, w)
        assert ((zc[1:-1] == 0).all(0)).sum() >= 8 and (zc[0] > 0).all()
