"""``daam_joint_tap_accumulate`` (include/daam_joint_tap.h) on the device, through ctypes on guarded buffers and through
``daam_amd.trace_joint``, held to the float64 reference of ``_joint_domain`` inside the bound derived there: every entry of every
plane, absolutely.

A statistics block is 128 query rows, an output tile 64 text rows x 128 cells, a key step 64 (two MFMA steps of 32): P = 1, 5, 63,
65 sit inside one block on either side of the key step of the image keys, 130 and 257 give two and three blocks with partial last
ones; T = 1, 7, 64, 77 sit on either side of one text tile, 154 and 333 give three and six with partial last ones.  Figures of every
case are printed before they are asserted (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _joint_domain as J
import _mmdit_standin as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _guarded(n_bytes, fill, offset=0):
    """A uint8 device buffer of ``n_bytes`` at ``offset`` bytes past 16-byte alignment, between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16) + offset
    raw[start:start + n_bytes] = fill
    return raw, start


def _put(buf, array):
    raw, start = buf
    flat = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).to(DEV)
    raw[start:start + flat.numel()] = flat


def _get(buf, n_bytes, dtype, shape):
    raw, start = buf
    return raw[start:start + n_bytes].cpu().numpy().view(dtype).reshape(shape).copy()


def _intact(buf, n_bytes):
    raw, start = buf
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


def _layout(x, dtype, layout):
    """``(uint16 memory image, (stride_b, stride_h, stride_row))`` of f32 [b, h, rows, d] in the layout of the projections
    ('interleaved', [b, rows, h d]) or packed [b, h, rows, d]."""
    b, h, rows, d = x.shape
    if layout == 'interleaved':
        return J.bits(x.transpose(0, 2, 1, 3), dtype), (rows * h * d, d, h * d)
    return J.bits(x, dtype), (h * rows * d, rows * d, d)


PLANE_GAP = 24                                        # floats between two planes of a per-head output: they must stay untouched


def accumulate_raw(calls, dtype, layout, per_head):
    """The chain ``calls`` of ``(q, k_txt, k_img, scale, weight)`` into one guarded ``sums`` pre-filled with NaN (the first call has
    ``accumulate == 0``), each with a workspace of exactly the bytes asked for: f32 [T, P] or [heads, T, P], after checking every
    guard, the gaps between planes and that the inputs are unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_joint()
    b, h, P, d = calls[0][0].shape
    T = calls[0][1].shape[2]
    planes, stride = (h, T * P + PLANE_GAP) if per_head else (1, 0)
    n_sums = 4 * ((planes - 1) * stride + T * P)
    sums = _guarded(n_sums, 0xFF, 4)
    assert np.isnan(_get(sums, n_sums, np.float32, (-1,))).all()
    for n, (q, kt, ki, scale, weight) in enumerate(calls):
        Pk = ki.shape[2]
        need = lib.daam_joint_tap_workspace(b, h, P)
        assert need >= 8 * b * h * P and need % 8 == 0
        images = dict(q=_layout(q, dtype, layout), kt=_layout(kt, dtype, layout), ki=_layout(ki, dtype, layout))
        bufs = {key: _guarded(max(im.nbytes, 16), 0) for key, (im, _) in images.items()}
        bufs['ws'] = _guarded(need, 0x5A, 8)
        for key, (im, _) in images.items():
            _put(bufs[key], im)
        before = {key: bufs[key][0].clone() for key in images}
        ptr = lambda key: bufs[key][0].data_ptr() + bufs[key][1]
        nat.check_joint(lib.daam_joint_tap_accumulate(
            ptr('q'), ptr('kt'), ptr('ki') if Pk else None, J.DAAM_F16 if dtype == 'f16' else J.DAAM_BF16, b, h, P, T, Pk, d,
            *images['q'][1], *images['kt'][1], *images['ki'][1], scale, weight, int(n > 0), sums[0].data_ptr() + sums[1], stride, ptr('ws'),
            need, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert all(_intact(bufs[key], max(images[key][0].nbytes, 16)) for key in images) and _intact(bufs['ws'], need) and _intact(sums, n_sums)
        assert all(torch.equal(bufs[key][0], before[key]) for key in before), 'an input changed'
    flat = _get(sums, n_sums, np.float32, (-1,))
    if not per_head:
        return flat.reshape(T, P)
    for p in range(planes - 1):
        gap = flat[p * stride + T * P:(p + 1) * stride]
        assert np.isnan(gap).all(), 'the floats between two planes were written'
    return np.stack([flat[p * stride:p * stride + T * P].reshape(T, P) for p in range(planes)])


def _report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f'\n{name}: worst error {err.max():.3e} bound there {float(bound.ravel()[(err / bound).argmax()]):.3e} worst device/bound {ratio:.3f}')
    return err, ratio


@pytest.mark.parametrize('case', J.CASES, ids=[J.case_id(c) for c in J.CASES])
def test_one_call_is_within_the_bound(case):
    P, T, Pk, d, dtype, (batch, heads), layout, per_head, regime = case
    q, kt, ki, scale = J.case_inputs(case)
    calls = [(q, kt, ki, scale, 1.0)]
    got = accumulate_raw(calls, dtype, layout, per_head)
    assert np.array_equal(got.view(np.uint32), accumulate_raw(calls, dtype, layout, per_head).view(np.uint32)), 'a second run'
    want, bound = J.reference_sums(calls, per_head), J.sums_bound(calls, per_head)
    err, ratio = _report(f'joint tap {J.case_id(case)}', got, want, bound)
    assert got.shape == want.shape and np.isfinite(got).all() and (err <= bound).all(), f'{ratio:.3f} of the bound'
    s_plane = batch if per_head else batch * heads
    if regime == 'zero_q':
        # raw = 0: every exp2 is 1, l = T + Pk exactly; 1 / l, s_plane fmas, the last fma and the rounding of the quotient itself
        assert np.abs(got - np.float32(s_plane / (T + Pk))).max() <= (s_plane + 3) * J.U * s_plane / (T + Pk)
    if Pk == 0:
        text_only = J.reference_text_only(q, kt, scale)
        plane = got.astype(np.float64).sum(axis=0) if per_head else got
        assert (np.abs(plane - text_only) <= (bound.sum(axis=0) if per_head else bound)).all(), 'Pk = 0 is the text-only softmax'
        assert np.abs(plane.sum(axis=0) - batch * heads).max() <= (bound.sum(axis=0) if per_head else bound).sum(axis=0).max() + T * J.U * batch * heads


@pytest.mark.parametrize('P,T,d,dtype,layout,per_head', [(65, 77, 64, 'f16', 'interleaved', False), (130, 154, 128, 'bf16', 'packed', True),
                                                        (257, 333, 64, 'f16', 'interleaved', True)])
def test_two_calls_accumulate_and_a_negative_weight(P, T, d, dtype, layout, per_head):
    q1, kt1, ki1, scale = J.inputs('small', 1, 3, P, T, P, d, dtype, seed=1)
    q2, kt2, ki2, _ = J.inputs('outlier', 1, 3, P, T, P, d, dtype, seed=2)
    for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
        calls = [(q1, kt1, ki1, scale, w1), (q2, kt2, ki2, scale, w2)]
        got = accumulate_raw(calls, dtype, layout, per_head)
        want, bound = J.reference_sums(calls, per_head), J.sums_bound(calls, per_head)
        err, ratio = _report(f'two calls P={P} T={T} d={d} {dtype} weights {w1} {w2}', got, want, bound)
        assert (err <= bound).all(), f'{ratio:.3f} of the bound'


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,size,grid', [(torch.float16, {}, (8, 8)), (torch.bfloat16, dict(height=96, width=160), (6, 10))])
def test_the_stand_in_pipeline_for_two_steps(dtype, size, grid):
    """A trace of the stand-in MMDiT pipeline: the sums are the float64 sum over the tapped calls (fed the projections the model itself
    recorded) inside the chained bound, the model's outputs are bit-equal to the untraced ones, per-head planes add up to the single
    plane, and the heat map composes with ``compute_word_heat_map`` and ``segment``."""
    import daam_amd
    steps, cells = 2, grid[0] * grid[1]
    pipe = M.make_pipe(device=DEV, dtype=dtype, seed=3)
    recorded = M.record(pipe)
    pipe(PROMPT, num_inference_steps=steps, **size)
    plain = [o.clone() for o in pipe.outputs]
    M.record(pipe, on=False)
    results = {}
    for per_head in (False, True):
        with daam_amd.trace_joint(pipe, per_head=per_head, **size) as tc:
            pipe(PROMPT, num_inference_steps=steps, **size)
            assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
            results[per_head] = (tc.state.sums.cpu().numpy(), tc.raw_heat_maps(), tc.compute_global_heat_map(), tc.state)
            if per_head:
                head_maps = tc.compute_head_heat_maps()
    T = M.CLIP_ROWS + M.T5_ROWS
    calls = [(q, kt, ki, scale, 1.0) for q, kt, ki, scale in recorded]
    assert len(calls) == 3 * steps and all(c[0].shape == (1, 2, cells, 64) and c[1].shape == (1, 2, T, 64) for c in calls)
    for per_head in (False, True):
        sums, raw, ghm, state = results[per_head]
        assert state.calls == len(calls) and state.slices == 2 * len(calls) and state.grid == grid
        want, bound = J.reference_sums(calls, per_head), J.sums_bound(calls, per_head)
        err, ratio = _report(f'stand-in MMDiT {grid[0]} x {grid[1]} {dtype} per_head={per_head}', sums, want, bound)
        assert sums.shape == want.shape and (err <= bound).all(), f'{ratio:.3f} of the bound'
        assert raw.shape == (T, *grid) and ghm.heat_maps.shape == (77, *grid) and ghm.heat_maps.dtype == torch.float32
    one, heads = results[False][0].astype(np.float64), results[True][0].astype(np.float64)
    both = J.sums_bound(calls) + J.sums_bound(calls, True).sum(axis=0)
    assert (np.abs(heads.sum(axis=0) - one) <= both).all(), 'per-head planes sum to the single plane'
    assert head_maps.shape == (2, T, *grid)
    ghm = results[False][2]
    assert torch.allclose(ghm.heat_maps.sum(dim=0).cpu(), torch.from_numpy(one[:77].sum(axis=0) / results[False][3].slices).float().view(*grid),
                          rtol=1e-5, atol=0)
    from daam_amd.utils import compute_token_merge_indices
    word = ghm.compute_word_heat_map('bicycle')
    idxs = compute_token_merge_indices(pipe.tokenizer, PROMPT, 'bicycle', None)[0]
    assert tuple(word.heatmap.shape) == grid
    assert np.allclose(word.heatmap.cpu().numpy().reshape(-1), one[idxs].mean(axis=0) / results[False][3].slices, rtol=1e-5, atol=0)

    class _Image:
        size = (grid[1] * 16, grid[0] * 16)
    seg = ghm.segment(['monkey', 'bicycle'], _Image(), threshold=0.5)
    assert seg.masks.shape[0] == 2 and seg.masks.shape[-2] * seg.masks.shape[-1] == cells * 256
