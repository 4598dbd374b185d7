"""The window-range tests' own footing, without a GPU (``tests/_bins_domain.py`` states the bound; ``tests/test_gpu_bins_domain.py`` holds
``daam_finalize_bins`` to it): the numpy emulation of ``finalize_bin_sum_kernel`` followed by the float64 finalize meets the bound on
every plane kind and shape of the GPU file, each mutant of the emulation misses it on a named case, and the check that held the
reduction before (one ``2e-6 * max(1, max |want|)`` over all rows, sides 16 / 32 / 64 / 128) is shown to see two of the mutants
differently: it cannot see a dropped tail at all, and it does see the token-stride mix-up."""
import numpy as np
import pytest

import _bins_domain as bd
import _finalize_domain as fd
from oracle import heatmap_oracle as ho


def _group(planes, spec, dtype, keys, b0, b1, rows, mutant=None):
    return bd.emulate_group(planes, spec['sides'], spec['heads'], dtype, spec['out_side'], keys, b0, b1, rows, mutant, spec['offset'])


def _layer_addrs(spec, dtype):
    return [4096 + spec['offset'] * bd.ELEM[dtype]] * len(spec['sides'])


@pytest.mark.parametrize('dtype', bd.DTYPES)
@pytest.mark.parametrize('name', list(bd.CUT_SETS))
def test_cut_piece_sets_meet_the_bound_and_reach_their_branches(name, dtype):
    """Every cut-piece set x plane kind x rows in {1, 5, 77}, windows [0, 3): the emulation meets the bound with the exact finalize
    (no MFMA floor), and the set reaches the branches of the reduction its table entry names, at every row count."""
    spec = bd.CUT_SETS[name]
    keys = bd.key_table(spec['sides'], spec['heads'])
    for rows in bd.ROWS:
        got = bd.branches(spec['sides'], spec['heads'], dtype, _layer_addrs(spec, dtype), keys, 0, bd.CUT_NB, rows)
        assert got == spec['reaches'][bd.ELEM[dtype]], (name, dtype, rows, got)
    for kind in bd.KINDS:
        planes = bd.native_windows(spec['sides'], kind, bd.CUT_NB, spec['heads'], dtype)
        for rows in bd.ROWS:
            want, allowance, exact = bd.reference(planes, spec['sides'], spec['out_side'], keys, 0, bd.CUT_NB, rows)
            if kind == 'exact':
                assert exact                                                 # the f32 sum IS the float64 sum
                allowance = 0 * allowance
            ratio, rel = bd.check(_group(planes, spec, dtype, keys, 0, bd.CUT_NB, rows), want, allowance, False,
                                  f'{name} {dtype} {kind} rows={rows}')
            print(f'{name} {dtype} {kind} rows={rows}: emulation, err_t/bound_t <= {ratio:.3f}, err_t/rowmax_t <= {rel:.3e}')


@pytest.mark.parametrize('dtype', bd.DTYPES)
@pytest.mark.parametrize('kind', bd.KINDS)
def test_window_counts_meet_the_bound(kind, dtype):
    """2, 7 and 50 windows of a 50-window context, sides 32 + 64: the in-order f32 sum stays inside (n_win - 1) * 2^-24 * W * S_t; on
    ``exact`` planes it has no error at all.  fp16 sums: the summed planes stay inside the MFMA routes' domain."""
    planes = bd.native_windows(bd.COUNT_SIDES, kind, bd.COUNT_NB, bd.COUNT_HEADS, dtype)
    spec = dict(sides=bd.COUNT_SIDES, heads=bd.COUNT_HEADS, out_side=64, offset=0)
    keys = bd.key_table(bd.COUNT_SIDES, bd.COUNT_HEADS)
    assert sum(float(np.abs(p.astype(np.float64)).sum(0).max()) for p in planes) <= fd.DOMAIN_MAX
    for b0, b1 in bd.COUNT_RANGES:
        want, allowance, exact = bd.reference(planes, bd.COUNT_SIDES, 64, keys, b0, b1, bd.TOKENS)
        if kind == 'exact':
            assert exact
            allowance = 0 * allowance
        ratio, rel = bd.check(_group(planes, spec, dtype, keys, b0, b1, bd.TOKENS), want, allowance, False, f'{kind} {dtype} [{b0}, {b1})')
        print(f'{kind} {dtype} windows [{b0}, {b1}): emulation, err_t/bound_t <= {ratio:.3f}, err_t/rowmax_t <= {rel:.3e}')


# mutant -> the named case that has to catch it: (cut-piece set or 'count', sums' dtype, plane kind, (b0, b1), rows)
KILLS = {
    'skip_last': ('count', 'float32', 'exact', (10, 17), 77),
    'short_stride': ('s6_12_24', 'bfloat16', 'exact', (0, 3), 5),
    'sum_in_dtype': ('count', 'float16', 'levelled', (0, 50), 77),
    'drop_tail': ('s6_12_h2', 'float16', 'levelled', (0, 3), 5),
    'token_stride': ('s6_12_24', 'float16', 'levelled', (0, 3), 5),
}


def _named(case):
    name, dtype, kind, (b0, b1), rows = case
    spec = dict(sides=bd.COUNT_SIDES, heads=bd.COUNT_HEADS, out_side=64, offset=0) if name == 'count' else bd.CUT_SETS[name]
    nb = bd.COUNT_NB if name == 'count' else bd.CUT_NB
    planes = bd.native_windows(spec['sides'], kind, nb, spec['heads'], dtype)
    keys = bd.key_table(spec['sides'], spec['heads'])
    want, allowance, exact = bd.reference(planes, spec['sides'], spec['out_side'], keys, b0, b1, rows)
    if kind == 'exact':
        assert exact
        allowance = 0 * allowance
    return spec, planes, keys, want, allowance


@pytest.mark.parametrize('mutant', bd.MUTANTS)
def test_each_mutant_misses_the_bound_on_its_named_case(mutant):
    """The bound is allowed the MFMA floor here, as the GPU case of the same name may be: a mutant has to break the WIDER bound."""
    case = KILLS[mutant]
    spec, planes, keys, want, allowance = _named(case)
    _, dtype, _, (b0, b1), rows = case
    mfma = 32 in spec['sides'] and spec['out_side'] == 64
    assert not bd.misses(_group(planes, spec, dtype, keys, b0, b1, rows), want, allowance, mfma)
    got = _group(planes, spec, dtype, keys, b0, b1, rows, mutant)
    err, rowmax = fd.row_errors(got, want)
    over = err / np.maximum(bd.bound(rowmax, allowance, mfma), 1e-300)
    print(f'mutant {mutant}: killed by {case}, worst err_t / bound_t = {over.max():.3g} on {int((over > 1).sum())} of {rows} rows')
    assert bd.misses(got, want, allowance, mfma), (mutant, case)


def test_f32_sums_carried_in_their_dtype_are_the_kernel():
    """``sum_in_dtype`` on f32 sums is no mutant: bit for bit the emulation (why its named case has fp16 sums)."""
    spec = bd.CUT_SETS['s6_12_24']
    planes = bd.native_windows(spec['sides'], 'signed', bd.CUT_NB, spec['heads'], 'float32')
    keys = bd.key_table(spec['sides'], spec['heads'])
    assert np.array_equal(_group(planes, spec, 'float32', keys, 0, 3, 5), _group(planes, spec, 'float32', keys, 0, 3, 5, 'sum_in_dtype'))


# ---- the check the reduction had before: tests/test_gpu_time_bins.py::test_finalize_bins_abi_against_numpy ---------------------------
OLD_SIDES, OLD_HEADS, OLD_NB = (16, 32, 64, 128), 3, 5
OLD_GROUPS = [(0, 5, 77), (1, 3, 12), (0, 2, 5), (2, 5, 30), (1, 4, 9), (0, 5, 20)]          # its window ranges (b0, b1, rows), all keys


def _old_check(got_planes, want_planes, rows):
    """Its reference (f32 bicubic -> clamp -> mean of the float64 window sums) and its verdict: one absolute bound over all rows."""
    def fin(planes):
        total = 0
        for side, p in planes:
            total = total + np.maximum(ho.bicubic_resize(p.reshape(rows, side, side).astype(np.float32), 64, np.float32), 0)
        return total * np.float32(1.0 / len(planes))
    want = fin(want_planes)
    err = float(np.abs(fin(got_planes) - want).max())
    return err, 2e-6 * max(1.0, float(np.abs(want).max()))


def test_what_the_old_check_sees_of_the_two_layout_mutants():
    """The old shapes (sides 16 / 32 / 64 / 128, three heads, uniform planes in [-0.5, 3.5), fp16 sums) under the old bound.

    ``drop_tail``: every ``rows * hw`` there is a multiple of 256, so no task has a cut piece and the mutant IS the kernel: error ratio
    0 of a bound of 2e-6 * max -- the margin is the whole bound, the check cannot fail.  ``token_stride``: at 77 rows it is the kernel
    as well (margin: the whole bound); at fewer rows it reads other tokens of other heads, uniform numbers of the same size, and the old
    check DOES reject it (errors of the order of the planes, 10^5 times its bound) -- what it never had is a cropped task on a side
    whose pixel count is no multiple of 8, which the cut-piece sets add."""
    rng = np.random.default_rng(7)
    planes = [(rng.random((OLD_NB, OLD_HEADS, 77, s * s)).astype(np.float32) * 4 - 0.5).astype(np.float16) for s in OLD_SIDES]
    keys = bd.key_table(OLD_SIDES, OLD_HEADS)
    seen = {}
    for b0, b1, rows in OLD_GROUPS:
        tasks = [(l, bd.plan_task(OLD_SIDES[l], OLD_HEADS, 'float16', 4096, h, b0, b1, rows)) for l, h in keys]
        assert all(bd.branch_of(t, 'float16') == 'pieces' for _, t in tasks)                  # no cut piece, no unaligned key
        want = [(OLD_SIDES[l], planes[l][b0:b1, h, :rows].astype(np.float64).sum(0)) for l, h in keys]
        for mutant in (None, 'drop_tail', 'token_stride'):
            got = [(OLD_SIDES[l], bd.emulate_task(planes[l].reshape(-1), t, 'float16', mutant)) for l, t in tasks]
            err, lim = _old_check(got, want, rows)
            seen[mutant, rows] = err / lim
    print('old check, err / bound per (mutant, rows):', {k: f'{v:.3g}' for k, v in seen.items()})
    assert all(v <= 1 for (m, _), v in seen.items() if m in (None, 'drop_tail'))
    assert seen['drop_tail', 5] == seen[None, 5] and seen['drop_tail', 77] == seen[None, 77]
    assert seen['token_stride', 77] == seen[None, 77] <= 1
    assert all(v > 1 for (m, rows), v in seen.items() if m == 'token_stride' and rows < 77)


def test_generator_windows():
    """Window b at 2^-(4 * (b % 6)); the unconditional half zero; ``exact`` numbers are multiples of 2^-10 below 2^6 in every dtype, and
    64 of them add up exactly in f32."""
    w = bd.draw_windows((8,), 'levelled', 7, 2)[0]
    assert w.shape == (7, 4, 64, 77) and not w[:, :2].any()
    med = np.median(np.abs(w[:, 2:, :, 0]), axis=(1, 2))
    np.testing.assert_allclose(np.log2(med), [-4.0 * (b % 6) for b in range(7)], atol=0.5)
    assert bd.draw_windows((8,), 'signed', 2, 2)[0].min() < 0
    for dtype in bd.DTYPES:
        (p,) = bd.native_windows((8,), 'exact', 64, 1, dtype)
        assert p.shape == (64, 1, 77, 64)
        q = p.astype(np.float64) / bd.EXACT_GRID
        assert np.array_equal(q, np.round(q)) and 0 < np.abs(p.astype(np.float64)).max() < bd.EXACT_TOP
        acc = np.zeros(p.shape[1:], np.float32)
        for b in range(64):
            acc = acc + p[b].astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), p.astype(np.float64).sum(0))
        assert (np.abs(p.astype(np.float64)).max((0, 1, 3)) > 0).sum() >= 30           # at least 30 of the 77 token rows are live
