"""``daam_amd.trace_flux`` (daam_amd/flux.py) on the device, on the stand-in FLUX pipeline of ``_flux_standin``: the
traced generation is bit-identical to the untraced one, the calls are counted by kind, and the sums lie inside the bound that
``_joint_domain`` derives for the joint tap (imported and not edited) against its float64 reference, which is fed the
post-rotary, dtype-rounded Q and K that the model's own processor recorded -- so a rotary pass that differed from the model's in one
bit of one element would feed the tap other inputs than the reference's.  Figures are printed before they are asserted."""
import numpy as np
import pytest
import torch

import _flux_standin as FS
import _joint_domain as J

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PROMPT = 'a dog and a dogs bench'
SHAPES = [(torch.float16, 64, dict(height=128, width=128), (8, 8)), (torch.bfloat16, 128, dict(height=96, width=160), (6, 10))]
STEPS = 2

_PLAIN = {}


def _plain(dtype, d, size):
    """The untraced generation of a shape, once: ``(pipe, outputs, recorded calls)``."""
    key = (dtype, d)
    if key not in _PLAIN:
        pipe = FS.make_pipe(device=DEV, dtype=dtype, seed=3, dim_head=d)
        recorded = FS.record(pipe)
        pipe(PROMPT, num_inference_steps=STEPS, **size)
        outputs = [o.clone() for o in pipe.outputs]
        FS.record(pipe, on=False)
        _PLAIN[key] = (pipe, outputs, tuple(recorded))
    return _PLAIN[key]


def _calls(recorded, blocks):
    return [(q, kt, ki, scale, 1.0) for kind, q, kt, ki, scale in recorded if blocks in ('all', kind)]


def _report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f'\n{name}: worst error {err.max():.3e} bound there {float(bound.ravel()[(err / bound).argmax()]):.3e} worst device/bound {ratio:.3f}')
    return err, ratio


@pytest.mark.parametrize('blocks', ['all', 'double', 'single'])
@pytest.mark.parametrize('dtype,d,size,grid', SHAPES, ids=['f16-d64-8x8', 'bf16-d128-6x10'])
def test_the_stand_in_pipeline_for_two_steps(dtype, d, size, grid, blocks):
    import daam_amd
    pipe, plain, recorded = _plain(dtype, d, size)
    cells, T = grid[0] * grid[1], FS.T5_ROWS
    assert [r[0] for r in recorded] == ['double', 'double', 'single', 'single'] * STEPS
    assert all(r[1].shape == (1, 2, cells, d) and r[2].shape == (1, 2, T, d) and r[3].shape == (1, 2, cells, d) for r in recorded)
    calls = _calls(recorded, blocks)
    expect = {'double': 2 * STEPS if blocks != 'single' else 0, 'single': 2 * STEPS if blocks != 'double' else 0}
    sums = {}
    for per_head in (False, True):
        with daam_amd.trace_flux(pipe, per_head=per_head, blocks=blocks, **size) as tc:
            assert tc.state is None and tc.grid == grid
            pipe(PROMPT, num_inference_steps=STEPS, **size)
            assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
            assert tc.calls_by_kind() == expect and tc.state.calls == len(calls) and tc.state.slices == 2 * len(calls)
            sums[per_head] = tc.state.sums.cpu().numpy()
            raw = tc.raw_heat_maps()
            assert raw.shape == (T, *grid) and raw.dtype == torch.float32
            if per_head:
                assert tc.compute_head_heat_maps().shape == (2, T, *grid)
            else:
                with pytest.raises(ValueError, match='per_head'):
                    tc.compute_head_heat_maps()
        want, bound = J.reference_sums(calls, per_head), J.sums_bound(calls, per_head)
        err, ratio = _report(f'stand-in FLUX {grid[0]} x {grid[1]} {dtype} d {d} blocks={blocks} per_head={per_head}', sums[per_head], want, bound)
        assert sums[per_head].shape == want.shape and (err <= bound).all(), f'{ratio:.3f} of the bound'
    both = J.sums_bound(calls) + J.sums_bound(calls, True).sum(axis=0)
    assert (np.abs(sums[True].astype(np.float64).sum(axis=0) - sums[False]) <= both).all(), 'per-head planes sum to the single plane'


def test_the_heat_map_is_over_t5_rows_and_composes():
    import daam_amd
    from daam_amd.utils import compute_token_merge_indices
    dtype, d, size, grid = SHAPES[0]
    pipe, plain, recorded = _plain(dtype, d, size)
    T = FS.T5_ROWS
    with daam_amd.trace_flux(pipe, **size) as tc:
        with pytest.raises(RuntimeError, match='No heat maps'):
            tc.compute_global_heat_map()
        pipe('a photo', prompt_2=PROMPT, num_inference_steps=1, **size)
        assert tc.last_prompt == PROMPT and pipe.checked[-1] == ('a photo', PROMPT), 'T5 encodes prompt_2 where it is given'
        raw, ghm, slices = tc.raw_heat_maps(), tc.compute_global_heat_map(), tc.state.slices
        first = raw.clone()
        pipe(PROMPT, num_inference_steps=1, **size)
        assert tc.calls_by_kind() == {'double': 2, 'single': 2} and torch.equal(tc.raw_heat_maps(), first), 'a new generation starts over'
        with pytest.raises(ValueError, match='single prompt'):
            pipe([PROMPT, PROMPT], num_inference_steps=1, **size)
    maps = ghm.heat_maps
    assert maps.shape == (1 + T, *grid) and maps.dtype == torch.float32 and not maps[0].any() and isinstance(ghm.tokenizer, daam_amd.T5RowTokenizer)
    assert ghm.tokenizer.tokenizer is pipe.tokenizer_2 and ghm.prompt == PROMPT
    assert torch.allclose(maps[1:], raw / slices, rtol=1e-6, atol=0)
    assert compute_token_merge_indices(ghm.tokenizer, PROMPT, 'dogs')[0] == [5, 6]
    one = maps.cpu().numpy().reshape(1 + T, -1)
    for word, rows in (('dog', [2]), ('dogs', [5, 6]), ('bench', [7])):
        got = ghm.compute_word_heat_map(word).heatmap.cpu().numpy().reshape(-1)
        assert np.allclose(got, one[rows].mean(axis=0), rtol=1e-5, atol=0), word
    with pytest.raises(ValueError, match='not found'):
        ghm.compute_word_heat_map('cat')

    class _Image:
        size = (grid[1] * 16, grid[0] * 16)
    seg = ghm.segment(['dog', 'bench'], _Image(), threshold=0.5)
    assert seg.masks.shape[0] == 2 and seg.masks.shape[-2] * seg.masks.shape[-1] == grid[0] * grid[1] * 256


def test_calls_that_do_not_fit_are_left_alone():
    import daam_amd
    dtype, d, size, grid = SHAPES[0]
    pipe, plain, recorded = _plain(dtype, d, size)
    try:
        with daam_amd.trace_flux(pipe, height=96, width=160) as tc:              # 60 cells; the generation has 64
            pipe(PROMPT, num_inference_steps=1, **size)
            assert tc.calls_by_kind() == {'double': 0, 'single': 0} and tc.state is None, 'another row count is not tapped'
            assert torch.equal(pipe.outputs[0], plain[0])
        with daam_amd.trace_flux(pipe, height=192, width=192, blocks='single') as tc:      # 144 cells: fewer rows than cells + 1
            pipe(PROMPT, num_inference_steps=1, **size)
            assert tc.calls_by_kind() == {'double': 0, 'single': 0} and tc.state is None
        with daam_amd.trace_flux(pipe, **size) as tc:
            pipe.mask_fn = lambda n: torch.zeros(n, n, dtype=dtype, device=DEV)
            pipe(PROMPT, num_inference_steps=1, **size)
            assert tc.calls_by_kind() == {'double': 0, 'single': 0} and tc.state is None, 'a masked call is not tapped'
            pipe.mask_fn = None
            pipe.batch = 2
            with pytest.raises(ValueError, match='one prompt, one image per prompt'):
                pipe(PROMPT, num_inference_steps=1, **size)
    finally:
        pipe.mask_fn, pipe.batch = None, 1


@pytest.mark.parametrize('dtype,d,size,grid', SHAPES, ids=['f16-d64-8x8', 'bf16-d128-6x10'])
def test_no_rotary_table_taps_the_projections_and_a_table_of_another_layout_is_converted_once(dtype, d, size, grid):
    import daam_amd
    pipe, plain, recorded = _plain(dtype, d, size)
    try:
        pipe.rotary = False
        unrotated = FS.record(pipe)
        with daam_amd.trace_flux(pipe, **size) as tc:
            pipe(PROMPT, num_inference_steps=1, **size)
            assert tc.calls_by_kind() == {'double': 2, 'single': 2} and tc._rotated is None and len(tc.table) == 0, 'no rotary pass'
            sums = tc.state.sums.cpu().numpy()
        FS.record(pipe, on=False)
        calls = _calls(unrotated, 'all')
        assert len(calls) == 4 and not np.array_equal(calls[0][0], recorded[0][1]), 'the model itself ran without the rotation'
        err, ratio = _report(f'no rotary {dtype} d {d}', sums, J.reference_sums(calls), J.sums_bound(calls))
        assert (err <= J.sums_bound(calls)).all(), f'{ratio:.3f} of the bound'
        pipe.rotary, pipe.table_layout = True, 'columns'
        with daam_amd.trace_flux(pipe, **size) as tc:
            pipe(PROMPT, num_inference_steps=STEPS, **size)
            assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs))
            assert len(tc.table) == 2, 'cos and sin went through .float().contiguous() once for the 8 tapped calls'
            sums = tc.state.sums.cpu().numpy()
        calls = _calls(recorded, 'all')
        err, ratio = _report(f'converted table {dtype} d {d}', sums, J.reference_sums(calls), J.sums_bound(calls))
        assert (err <= J.sums_bound(calls)).all(), f'{ratio:.3f} of the bound'
    finally:
        pipe.rotary, pipe.table_layout = True, 'rows'
        FS.record(pipe, on=False)
