"""The oracle, the bound and the cases of ``tests/test_gpu_region_scores.py`` hold what that file relies on (no GPU): the float64
oracle of ``tests/_region_domain.py`` is the masked sum of ``F.interpolate(mode='bicubic')``, a footprint sums to its mask's area, the
f32 emulation of the kernels meets the bound on every case and each of six mutants misses it on some case, the count of roundings
stays under the issue's cap, and the feature is declared on every layer (header, ctypes table, build list, Python API)."""
import functools
import os
import re

import numpy as np
import pytest

import _region_domain as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(sizes, n, first):
    (h, w), (H, W) = sizes
    masks, maps = rd.mask_stack(H, W, n, first), rd.map_sets(h, w)
    return masks, maps, rd.oracle(masks, maps, h, w)


@pytest.mark.parametrize('sizes', rd.SIZE_SETS, ids=str)
def test_oracle_is_the_masked_sum_of_the_bicubic_resize(sizes):
    """want = sum under the mask of F.interpolate(bicubic, align_corners=False) in float64, within the gap between f32 and float64
    coefficients: 3 * 2^-24 * max|src| per weight, i.e. that much of sum |w| |v| over the 16 taps of every set pixel."""
    import torch
    import torch.nn.functional as F
    (h, w), (H, W) = sizes
    n = 3
    masks, maps, ref = _case(sizes, n, 0)
    v = torch.from_numpy(maps[:, :, None].astype(np.float64).reshape(-1, 1, h, w))
    if (H, W) == (h, w):
        big = v
    else:
        big = F.interpolate(v, size=(H, W), mode='bicubic', align_corners=False)
    big = big.reshape(maps.shape[0], maps.shape[1], H, W).numpy()
    got = np.einsum('myx,gtyx->gmt', (masks != 0).astype(np.float64), big)
    # a weight's error is <= 3 u max|src| in absolute terms (weights are O(1)): per set pixel 16 taps, two weights each
    per_weight = 3 * rd.U * max(h, w, 1)
    taps_mag = np.einsum('mij,gtij->gmt', rd.footprint64(masks, h, w)[1], np.abs(maps.astype(np.float64)))
    slack = 2 * per_weight * 1.25 * 4 * np.einsum('m,gt->gmt', ref['area'].astype(np.float64), np.abs(maps).max((2, 3)).astype(np.float64))
    assert (np.abs(got - ref['want']) <= slack + 1e-12 * taps_mag + 1e-300).all(), float(np.abs(got - ref['want']).max())


@pytest.mark.parametrize('sizes', rd.SIZE_SETS, ids=str)
def test_footprint_sums_to_the_area(sizes):
    """The weights of a pixel sum to 1 on each axis (to 2 u each in f32), so sum_ij F64[m] = area[m] within 4 u sum F_abs."""
    _, _, ref = _case(sizes, 3, 0)
    total, total_abs = ref['F64'].sum((1, 2)), ref['F_abs'].sum((1, 2))
    assert (np.abs(total - ref['area']) <= 4 * rd.U * total_abs).all()


@pytest.mark.parametrize('case', list(rd.cases()), ids=str)
def test_emulation_meets_the_bound(case):
    sizes, n, first = case
    (h, w), _ = sizes
    masks, maps, ref = _case(*case)
    scores, area, foot = rd.emulate(masks, maps, h, w)
    assert (area == ref['area']).all()
    assert rd.worst(scores, ref) <= 1.0, rd.worst(scores, ref)
    if sizes[0] == sizes[1]:
        assert (foot == (masks != 0).astype(np.float32)).all()
    clear = [i for i, k in enumerate(rd.stack_kinds(n, first)) if k == 'all_clear']
    assert (scores[:, clear] == 0).all() and (scores[-1, :, rd.ZERO_ROW] == 0).all()


MUTANT_CASES = [(((64, 64), (128, 128)), 3, 0), (((64, 64), (200, 333)), 3, 0), (((16, 24), (37, 53)), 3, 6), (((2, 2), (9, 9)), 3, 0),
                (((48, 48), (32, 32)), 3, 6)]


@pytest.mark.parametrize('mutant', rd.MUTANTS)
def test_every_mutant_misses_the_bound_somewhere(mutant):
    ratios = {}
    for case in MUTANT_CASES:
        (h, w), _ = case[0]
        masks, maps, ref = _case(*case)
        scores, area, _ = rd.emulate(masks, maps, h, w, mutant=mutant)
        ratios[str(case)] = np.inf if (area != ref['area']).any() else rd.worst(scores, ref)
    assert max(ratios.values()) > 1.0, ratios


def test_rounding_count_stays_under_the_cap():
    for sizes in rd.SIZE_SETS:
        (h, w), (H, W) = sizes
        K, parts = rd.roundings(rd.geometry(H, W, h, w))
        assert K * rd.U <= rd.CAP, (sizes, K, parts)
    K, parts = rd.roundings(rd.geometry(1024, 1024, 64, 64))
    assert (K, parts['x'], parts['y'], parts['combine'], parts['dot']) == (155, 88, 33, 3, 25), (K, parts)


def test_cell_ranges_cover_every_pixel_that_reaches_a_cell():
    """The integer ranges the x pass and the combine walk are supersets of what the f32 tables say, and the band window holds every
    cell row a band reaches."""
    pairs = {(n_in, n_out) for (h, w), (H, W) in rd.SIZE_SETS for n_in, n_out in ((h, H), (w, W))}
    pairs |= {(128, 1), (1, 1024), (3, 1000), (128, 129), (127, 128), (5, 4096), (100, 7)}
    for n_in, n_out in sorted(pairs):
        base, fold = rd.tables(n_in, n_out, False)
        weights = rd._dense32(base, fold, n_in)              # a slot past the taps (the low end clamped) holds no weight
        for j in range(n_in):
            lo, hi = rd.cell_range(j, n_out, n_in, 1)
            reach = np.flatnonzero(weights[:, j])
            assert reach.size == 0 or (lo <= reach[0] and reach[-1] < hi), (n_in, n_out, j)
    for (h, w), (H, W) in rd.SIZE_SETS + [((128, 5), (130, 40000)), ((7, 128), (4000, 3))]:
        g = rd.geometry(H, W, h, w)
        by, _ = rd.tables(h, H, (H, W) == (h, w))
        for y0 in range(0, H, g['band']):
            last = by[min(y0 + g['band'], H) - 1]
            assert min(last + 3, h - 1) - by[y0] < g['win'], (h, H, y0)


def test_the_feature_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, 'include', 'daam_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bsize_t\s+daam_region_scores_workspace\s*\(\s*int n_masks, int H, int W, int h, int w\s*\)', code)
    assert re.search(r'\bint\s+daam_region_scores\s*\(\s*const uint8_t\* masks, int n_masks, int H, int W,', code)
    assert re.search(r'#define\s+DAAM_ABI_VERSION\s+6\b', header)
    assert 'heatmap.py:77-93' in header and 'evaluate.py' in header
    from daam_amd import _native, build
    assert 'daam_region_scores' in _native.EXPORTS and 'daam_region_scores_workspace' in _native.EXPORTS
    assert _native.ABI_VERSION == 6
    assert 'daam_region_scores.hip' in build.SOURCES
    import daam_amd
    from daam_amd import engine, heatmap
    assert callable(heatmap.GlobalHeatMap.attribute) and callable(engine.region_scores)
    fields = set(heatmap.RegionAttribution.__dataclass_fields__)
    assert {'scores', 'area', 'footprint'} <= fields
    for name in ('mean', 'word_scores', 'top_words', 'cpu'):
        assert callable(getattr(heatmap.RegionAttribution, name))
    assert daam_amd.RegionAttribution is heatmap.RegionAttribution
