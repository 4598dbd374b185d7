"""The rectangular finalize tests' own footing, without a GPU (``tests/_rect_domain.py`` states the contract, the cases and the
emulation; ``tests/test_gpu_rect_domain.py`` holds the kernels to them): the float32 emulation of the kernel's own order stays inside
the contract on every case, so the reference alone does not use up the bound; the contract catches seven defects of a multi-key walk;
and ``plan_chunks`` gives the walks the cases are there for."""
import math

import numpy as np
import pytest

import _finalize_domain as fd
import _rect_domain as rd


def _runs(case):
    """(variant, k) of a case: the whole magnitude matrix on ``rd.MAGNITUDE_CASES``, k = 0 signed on the others."""
    if case in rd.MAGNITUDE_CASES:
        return [(v, k) for v in fd.VARIANTS for k in sorted(set(fd.K_EXACT + [40]))]
    return [('signed', 0)]


@pytest.mark.parametrize('dtype', fd.DTYPES)
@pytest.mark.parametrize('case', list(rd.CASES))
def test_emulation_within_the_contract(case, dtype):
    """The kernel's order in float32 against the float64 reference, with the chunk count the host would choose: every token row inside
    ``rel_bound(N) * rowmax_t``, at every magnitude the GPU test uses."""
    out_hw = rd.CASES[case]['out_hw']
    groups = rd.groups_of(case)
    worst = 0.0
    for variant, k in _runs(case):
        if k == 40 and dtype == 'float16':
            continue
        k, planes = rd.planes_at(case, variant, k, dtype)
        keys = rd.key_planes(planes)
        want = rd.reference(keys, out_hw, groups)
        got = rd.emulate_groups(keys, out_hw, groups)
        for g, (idx, rows) in enumerate(groups):
            assert got[g].shape == (rows,) + tuple(out_hw)
            worst = max(worst, rd.assert_contract(got[g], want[g], len(idx), f'{case} {dtype} {variant} k={k} group {g}'))
    n_chunks, _ = rd.plan_of(groups)
    print(f'\nRECTDOMAIN emulation {case} {dtype} | n_chunks {n_chunks}, {rd.keys_per_workgroup(groups)} keys per workgroup | '
          f'err_t/rowmax_t <= 2^{rd.log2(worst):.2f}')


def test_masked_and_short_runs_of_the_emulation():
    """The two further launches of the GPU test on ``multi_walk_single``: the 14-key mask (13 chunks) and ``n_rows = 5`` (24 chunks)."""
    _, planes = rd.planes_at('multi_walk_single', 'signed', 0, 'float32')
    keys = rd.key_planes(planes)
    for kw in (dict(key_mask=rd.KEY_MASK), dict(n_rows=5)):
        groups = rd.groups_of('multi_walk_single', **kw)
        (want,), (got,) = rd.reference(keys, (12, 20), groups), rd.emulate_groups(keys, (12, 20), groups)
        rd.assert_contract(got, want, len(groups[0][0]), str(kw))


@pytest.mark.parametrize('mutant', [m for m in rd.MUTANTS if m != 'inv_max_n'])
@pytest.mark.parametrize('variant', fd.VARIANTS)
def test_contract_catches_a_broken_walk(mutant, variant):
    """Each defect of the emulation on ``multi_walk_single`` (13 chunks, two keys per workgroup) leaves the contract.  The clamp
    mutants are judged on the signed planes only: on non-negative planes the clamp only removes bicubic undershoot."""
    if variant == 'nonneg' and mutant in ('no_clamp', 'clamp_after_mean'):
        variant = 'signed'
    _, planes = rd.planes_at('multi_walk_single', variant, 0, 'float32')
    keys = rd.key_planes(planes)
    groups = rd.groups_of('multi_walk_single')
    (want,) = rd.reference(keys, (12, 20), groups)
    (got,) = rd.emulate_groups(keys, (12, 20), groups, mutant)
    with pytest.raises(AssertionError, match='outside the contract'):
        rd.assert_contract(got, want, 24, mutant)


def test_contract_catches_the_largest_groups_factor():
    """``1 / max_n`` in place of a group's own ``1 / n``.  On a single map the two are the same number (checked: the mutant is the
    emulation, bit for bit, on ``multi_walk_single``), so this defect is judged where it exists: on ``unequal_groups``, whose group 0 has one
    key and whose largest group has five."""
    _, planes = rd.planes_at('multi_walk_single', 'signed', 0, 'float32')
    keys, groups = rd.key_planes(planes), rd.groups_of('multi_walk_single')
    np.testing.assert_array_equal(rd.emulate_groups(keys, (12, 20), groups, 'inv_max_n')[0], rd.emulate_groups(keys, (12, 20), groups)[0])
    _, planes = rd.planes_at('unequal_groups', 'signed', 0, 'float32')
    keys, groups = rd.key_planes(planes), rd.groups_of('unequal_groups')
    want, got = rd.reference(keys, (12, 20), groups), rd.emulate_groups(keys, (12, 20), groups, 'inv_max_n')
    with pytest.raises(AssertionError, match='outside the'):
        rd.assert_contract(got[0], want[0], 1, 'inv_max_n group 0')
    rd.assert_contract(got[1], want[1], 5, 'inv_max_n group 1')                   # the largest group's own factor


def test_plan_chunks_and_the_walks():
    """The chunk counts the cases are built on, and which key kinds meet in one workgroup."""
    assert rd.plan_chunks(24, 77) == 13 and rd.plan_chunks(2, 12 * 77) == 1 and rd.plan_chunks(5, 86) == min(5, (1024 + 43) // 86) == 5
    assert rd.plan_chunks(24, 5) == 24 and rd.plan_chunks(14, 77) == 13 and rd.plan_chunks(8, 77) == 8 and rd.plan_chunks(16, 77) == 13
    assert rd.plan_chunks(3, 5000) == 1                                            # never below one chunk
    expect = {'multi_walk_single': (13, 77 * 13, 2), 'one_chunk_groups': (1, 77 * 12, 2), 'unequal_groups': (5, 77 * 5 * 2, 1),
              'pieces_mix_16x24': (13, 77 * 13, 2), 'pieces_mix_14x6': (13, 77 * 13, 2), 'mixed_axes': (8, 77 * 8, 1)}
    for case, (n_chunks, grid, per) in expect.items():
        groups = rd.groups_of(case)
        assert rd.plan_of(groups) == (n_chunks, grid), case
        assert rd.keys_per_workgroup(groups) == per, case
    for case in ('multi_walk_single', 'one_chunk_groups', 'pieces_mix_16x24', 'pieces_mix_14x6'):
        groups = rd.groups_of(case)
        assert max(math.ceil(len(idx) / rd.plan_of(groups)[0]) for idx, _ in groups) >= 2, case
    assert rd.keys_per_workgroup(rd.groups_of('multi_walk_single', key_mask=rd.KEY_MASK)) == 2 and sum(rd.KEY_MASK) == 14
    assert rd.keys_per_workgroup(rd.groups_of('multi_walk_single', n_rows=5)) == 1
    # unequal_groups: group 0's single key sits in chunk 0, chunks 1 .. 4 walk nothing
    assert rd.walks(1, 5) == [[0], [], [], [], []]

    def met(case, dtype, groups=None):
        """The (kind of the earlier key, kind of the later key) pairs that follow each other in some workgroup."""
        shapes, out_hw = rd.key_shapes(case), rd.CASES[case]['out_hw']
        groups = groups or rd.groups_of(case)
        n_chunks, _ = rd.plan_of(groups)
        pairs = set()
        for idx, _ in groups:
            for walk in rd.walks(len(idx), n_chunks):
                for a, b in zip(walk, walk[1:]):
                    pairs.add((rd.key_kind(shapes[idx[a]], out_hw, dtype) + (shapes[idx[a]],), rd.key_kind(shapes[idx[b]], out_hw, dtype) + (shapes[idx[b]],)))
        return pairs
    for dtype in fd.DTYPES:
        kinds = {(a[0], b[0]) for a, b in met('multi_walk_single', dtype)}
        assert {('table', 'copy'), ('copy', 'table'), ('table', 'table')} <= kinds, kinds
        shapes = {(a[2], b[2]) for a, b in met('one_chunk_groups', dtype)}
        assert shapes == {((3, 5), (12, 20)), ((3, 5), (6, 10)), ((12, 20), (6, 10)), ((12, 20), (3, 5)), ((6, 10), (3, 5)), ((6, 10), (12, 20))}
        assert all(a[1] == b[1] == 'pieces' for a, b in met('pieces_mix_16x24', dtype))
        assert {(a[0], b[0]) for a, b in met('pieces_mix_14x6', dtype)} == {('table', 'copy')}
    assert {(a[1], b[1]) for a, b in met('pieces_mix_14x6', 'float16')} == {('elements', 'elements')}
    assert {(a[1], b[1]) for a, b in met('pieces_mix_14x6', 'float32')} == {('elements', 'pieces')}      # both load paths feed one tile
    # the 12 x 20 copy key: 240 elements, pieces in every dtype; 60 and 15 elements: element by element for 16-bit sums
    assert rd.key_kind((12, 20), (12, 20), 'float16') == ('copy', 'pieces') and rd.key_kind((6, 10), (12, 20), 'bfloat16') == ('table', 'elements')
    masked = {(a[2], b[2]) for a, b in met('multi_walk_single', 'float16', rd.groups_of('multi_walk_single', key_mask=rd.KEY_MASK))}
    assert masked == {((6, 10), (3, 5))}


def test_levels_and_reference_of_rectangular_planes():
    """Token rows 8 x apart per level; the signed variant signed; the reference of a key of the output's size is its clamp."""
    for variant in fd.VARIANTS:
        planes = rd.draw_planes('mixed_axes', variant)
        assert [p.shape for p in planes] == [(2, rd.TOKENS, 12, 10), (2, rd.TOKENS, 6, 20), (2, rd.TOKENS, 24, 40), (2, rd.TOKENS, 12, 30)]
        med = np.median(np.abs(planes[2]), axis=(0, 2, 3))
        np.testing.assert_allclose(np.log2(med), -fd.LEVEL_STEP * (np.arange(rd.TOKENS) % fd.N_LEVELS), atol=0.35)
        assert (planes[0].min() < 0) == (variant == 'signed')
    p = rd.draw_planes('multi_walk_single', 'signed')[1][0]
    np.testing.assert_array_equal(rd.global64([p], 12, 20), np.maximum(p.astype(np.float64), 0))
    # an axis of the output's size goes through the identity table in the kernel and is a copy in the reference: the same numbers
    q = rd.draw_planes('mixed_axes', 'signed')[0][0]
    (got,) = rd.emulate_groups([q], (12, 20), [([0], rd.TOKENS)])
    rd.assert_contract(got, rd.global64([q], 12, 20), 1, 'rows are a copy')
