"""``daam_joint_affinity_accumulate`` (include/daam_joint_affinity.h) on the device, through ctypes on guarded buffers
and through ``daam_amd.trace_joint`` / ``trace_flux`` with ``self_affinity=True``, held to the float64 reference of
``_joint_affinity_domain`` inside the bound derived there: every entry of the matrix, absolutely.  The statistics come from one
``daam_joint_tap_accumulate`` call on the same inputs, in a workspace of exactly the bytes asked for.

A tile of sums is 128 x 128, a wave's share 64 x 64, an MFMA block 32 x 32, a pass through LDS 64 of depth: P = 1, 5, 63, 65 sit
inside one tile on either side of a wave's share, 130 and 257 give two and three tiles a side with partial last ones; d = 128 takes
two passes.  Figures of every case are printed before they are asserted (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _flux_standin as FS
import _joint_affinity_domain as JA
import _mmdit_standin as M
from _joint_domain import bits
from oracle import fake_diffusers as fd

J = JA.J
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
        return bits(x.transpose(0, 2, 1, 3), dtype), (rows * h * d, d, h * d)
    return bits(x, dtype), (h * rows * d, rows * d, d)


def accumulate_raw(calls, dtype, layout, halve_rinv=False, with_text=False):
    """The chain ``calls`` of ``(q, k_txt, k_img, scale, weight)`` into one guarded ``sums`` pre-filled with NaN (the first call has
    ``accumulate == 0``): per call one joint tap that leaves the statistics in a guarded workspace of exactly the bytes asked for, then
    the affinity on them.  Returns f32 [P, Pk] (with ``with_text`` also the tap's [T, P] of the LAST call alone), after checking every
    guard and that q, k_img and the statistics are unchanged by the affinity call."""
    from daam_amd import _native as nat
    tap, lib = nat.load_joint(), nat.load_joint_affinity()
    b, h, P, d = calls[0][0].shape
    Pk = calls[0][2].shape[2]
    n_sums = 4 * P * Pk
    sums = _guarded(n_sums, 0xFF, 4)
    assert np.isnan(_get(sums, n_sums, np.float32, (-1,))).all()
    code = J.DAAM_F16 if dtype == 'f16' else J.DAAM_BF16
    stream = torch.cuda.current_stream().cuda_stream
    for n, (q, kt, ki, scale, weight) in enumerate(calls):
        T = kt.shape[2]
        need = lib.daam_joint_affinity_stats_bytes(b, h, P)
        assert need == tap.daam_joint_tap_workspace(b, h, P) == 8 * b * h * -(-P // 128) * 128
        images = dict(q=_layout(q, dtype, layout), kt=_layout(kt, dtype, layout), ki=_layout(ki, dtype, layout))
        bufs = {key: _guarded(max(im.nbytes, 16), 0) for key, (im, _) in images.items()}
        bufs['ws'] = _guarded(need, 0x5A, 8)
        bufs['text'] = _guarded(4 * T * P, 0xFF, 4)
        for key, (im, _) in images.items():
            _put(bufs[key], im)
        ptr = lambda key: bufs[key][0].data_ptr() + bufs[key][1]
        nat.check_joint(tap.daam_joint_tap_accumulate(ptr('q'), ptr('kt'), ptr('ki'), code, b, h, P, T, Pk, d, *images['q'][1], *images['kt'][1],
                                                      *images['ki'][1], scale, 1.0, 0, ptr('text'), 0, ptr('ws'), need, stream))
        if halve_rinv:
            torch.cuda.synchronize()
            stats = _get(bufs['ws'], need, np.float32, (-1, 2))
            stats[:, 1] *= np.float32(0.5)
            _put(bufs['ws'], stats)
        torch.cuda.synchronize()
        before = {key: bufs[key][0].clone() for key in ('q', 'ki', 'ws')}
        nat.check_joint_affinity(lib.daam_joint_affinity_accumulate(ptr('q'), ptr('ki'), ptr('ws'), need, code, b, h, P, Pk, d, *images['q'][1],
                                                                    *images['ki'][1], scale, weight, int(n > 0), sums[0].data_ptr() + sums[1],
                                                                    stream))
        torch.cuda.synchronize()
        assert all(_intact(bufs[key], max(images[key][0].nbytes, 16)) for key in images) and _intact(bufs['ws'], need) and _intact(sums, n_sums)
        assert all(torch.equal(bufs[key][0], before[key]) for key in before), 'an input or the statistics changed'
    out = _get(sums, n_sums, np.float32, (P, Pk))
    return (out, _get(bufs['text'], 4 * T * P, np.float32, (T, P))) if with_text else out


def _report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f'\n{name}: worst error {err.max():.3e} bound there {float(bound.ravel()[(err / bound).argmax()]):.3e} worst device/bound {ratio:.3f}')
    return err, ratio


@pytest.mark.parametrize('case', JA.CASES, ids=[JA.case_id(c) for c in JA.CASES])
def test_one_call_is_within_the_bound(case):
    P, T, Pk, d, dtype, (batch, heads), layout, regime = case
    q, kt, ki, scale = JA.case_inputs(case)
    calls = [(q, kt, ki, scale, 1.0)]
    got = accumulate_raw(calls, dtype, layout)
    assert np.array_equal(got.view(np.uint32), accumulate_raw(calls, dtype, layout).view(np.uint32)), 'a second run'
    want, bound = JA.reference_sums(calls), JA.sums_bound(calls)
    err, ratio = _report(f'joint affinity {JA.case_id(case)}', got, want, bound)
    assert got.shape == want.shape == (P, Pk) and np.isfinite(got).all() and (err <= bound).all(), f'{ratio:.3f} of the bound'
    if regime == 'zero_q':
        s = batch * heads
        assert np.abs(got - np.float32(s / (T + Pk))).max() <= (s + 3) * JA.U * s / (T + Pk)


@pytest.mark.parametrize('P,T,d,dtype,layout', [(65, 77, 64, 'f16', 'interleaved'), (130, 154, 128, 'bf16', 'packed')])
def test_two_calls_accumulate_and_a_negative_weight(P, T, d, dtype, layout):
    q1, kt1, ki1, scale = JA.inputs('small', 1, 3, P, T, P, d, dtype, seed=1)
    q2, kt2, ki2, _ = JA.inputs('outlier', 1, 3, P, T, P, d, dtype, seed=2)
    for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
        calls = [(q1, kt1, ki1, scale, w1), (q2, kt2, ki2, scale, w2)]
        got = accumulate_raw(calls, dtype, layout)
        want, bound = JA.reference_sums(calls), JA.sums_bound(calls)
        err, ratio = _report(f'two calls P={P} T={T} d={d} {dtype} weights {w1} {w2}', got, want, bound)
        assert (err <= bound).all(), f'{ratio:.3f} of the bound'


@pytest.mark.parametrize('P,T,d,dtype,layout', [(130, 77, 64, 'f16', 'interleaved'), (65, 154, 128, 'bf16', 'packed')])
def test_the_kernel_uses_the_statistics_it_is_given(P, T, d, dtype, layout):
    """1 / l halved on the device between the two calls: every entry is exactly half (a product by a power of two and a sum of halves
    are exact; nothing is near the subnormal range in the regime 'small')."""
    q, kt, ki, scale = JA.inputs('small', 2, 3, P, T, P, d, dtype, seed=3)
    calls = [(q, kt, ki, scale, 1.0)]
    whole, half = accumulate_raw(calls, dtype, layout), accumulate_raw(calls, dtype, layout, halve_rinv=True)
    assert whole.min() > 2.0 ** -100 and np.array_equal((np.float32(0.5) * whole).view(np.uint32), half.view(np.uint32))


@pytest.mark.parametrize('case', [c for c in JA.CASES if c[0] in (63, 130, 200)], ids=lambda c: JA.case_id(c))
def test_text_and_image_columns_add_up_to_the_slices(case):
    P, T, Pk, d, dtype, (batch, heads), layout, regime = case
    q, kt, ki, scale = JA.case_inputs(case)
    calls = [(q, kt, ki, scale, 1.0)]
    image, text = accumulate_raw(calls, dtype, layout, with_text=True)
    total = text.astype(np.float64).sum(axis=0) + image.astype(np.float64).sum(axis=1)
    slack = J.sums_bound(calls).sum(axis=0) + JA.sums_bound(calls).sum(axis=1)
    print(f'\ntotal probability {JA.case_id(case)}: worst {np.abs(total - batch * heads).max():.3e}, bound there {slack[np.abs(total - batch * heads).argmax()]:.3e}')
    assert (np.abs(total - batch * heads) <= slack).all()


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def _check_trace(tc_off, tc_on, plain, pipe, calls, grid, name):
    """What both front ends owe: counts, the chained bound, bit-identical planes and outputs, propagate through the heat map."""
    from daam_amd import engine as E
    planes_off, (planes_on, aff, ghm) = tc_off, tc_on
    assert torch.equal(planes_off, planes_on), 'the heat-map planes are bit-identical with the option on or off'
    assert aff.grid == grid and aff.calls == len(calls) and aff.slices == sum(c[0].shape[0] * c[0].shape[1] for c in calls)
    want, bound = JA.reference_sums(calls), JA.sums_bound(calls)
    err, ratio = _report(name, aff.sums.cpu().numpy(), want, bound)
    assert (err <= bound).all(), f'{ratio:.3f} of the bound'
    assert torch.allclose(aff.sums.sum(dim=1).cpu().double(), torch.from_numpy(aff.slices - JA.text_mass(calls)), rtol=1e-5, atol=0)
    out = ghm.propagate(aff, 2)
    assert torch.equal(out.heat_maps, E.affinity_propagate(aff.sums, ghm.heat_maps, 2))


@pytest.mark.parametrize('dtype,size,grid', [(torch.float16, {}, (8, 8)), (torch.bfloat16, dict(height=96, width=160), (6, 10))])
def test_the_stand_in_mmdit_for_two_steps(dtype, size, grid):
    import daam_amd
    steps = 2
    pipe = M.make_pipe(device=DEV, dtype=dtype, seed=3)
    recorded = M.record(pipe)
    pipe(PROMPT, num_inference_steps=steps, **size)
    plain = [o.clone() for o in pipe.outputs]
    M.record(pipe, on=False)
    with daam_amd.trace_joint(pipe, **size) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        off = tc.state.sums.clone()
        with pytest.raises(ValueError, match='self_affinity=True'):
            tc.compute_self_affinity()
    with daam_amd.trace_joint(pipe, self_affinity=True, **size) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
        on = (tc.state.sums.clone(), tc.compute_self_affinity(), tc.compute_global_heat_map())
    calls = [(q, kt, ki, scale, 1.0) for q, kt, ki, scale in recorded]
    assert len(calls) == 3 * steps
    _check_trace(off, on, plain, pipe, calls, grid, f'stand-in MMDiT {grid[0]} x {grid[1]} {dtype}')


@pytest.mark.parametrize('dtype,d,size,grid,blocks', [(torch.float16, 64, {}, (8, 8), 'all'), (torch.bfloat16, 128, dict(height=96, width=160), (6, 10), 'all'),
                                                     (torch.bfloat16, 128, dict(height=96, width=160), (6, 10), 'double'),
                                                     (torch.float16, 64, {}, (8, 8), 'single')])
def test_the_stand_in_flux_for_two_steps(dtype, d, size, grid, blocks):
    import daam_amd
    steps = 2
    kw = dict(height=size.get('height', FS.SIZE), width=size.get('width', FS.SIZE))
    pipe = FS.make_pipe(device=DEV, dtype=dtype, seed=2, dim_head=d)
    recorded = FS.record(pipe)
    pipe(PROMPT, num_inference_steps=steps, **size)
    plain = [o.clone() for o in pipe.outputs]
    FS.record(pipe, on=False)
    with daam_amd.trace_flux(pipe, blocks=blocks, **kw) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        off = tc.state.sums.clone()
    with daam_amd.trace_flux(pipe, blocks=blocks, self_affinity=True, **kw) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
        on = (tc.state.sums.clone(), tc.compute_self_affinity(), tc.compute_global_heat_map())
    calls = [(q, kt, ki, scale, 1.0) for kind, q, kt, ki, scale in recorded if blocks in ('all', kind)]
    assert len(calls) == (4 if blocks == 'all' else 2) * steps
    _check_trace(off, on, plain, pipe, calls, grid, f'stand-in FLUX {grid[0]} x {grid[1]} {dtype} d {d} blocks={blocks}')


def test_it_sharpens_the_block_structured_case():
    """3.22's construction carried to joint attention at 12 x 20: ``segment`` after ``propagate(aff, 2)`` beats ``segment`` before and
    equals what the float64 affinity gives."""
    from daam_amd import GlobalHeatMap, SelfAffinity, engine as E
    from daam_amd.utils import compute_token_merge_indices
    qk, kt, truth, plane = JA.block_case()
    h, w = JA.BLOCK_GRID
    x = torch.from_numpy(qk[0].transpose(1, 0, 2).reshape(1, h * w, -1)).to(DEV, torch.float16)
    t = torch.from_numpy(kt[0].transpose(1, 0, 2).reshape(1, JA.BLOCK_TEXT, -1)).to(DEV, torch.float16)
    tap, eng = E.JointTapState(h, w, JA.BLOCK_TEXT), E.JointAffinityState(h, w)
    tap.tap(x, t, x, 1, 64 ** -0.5)
    eng.tap(x, x, 1, 64 ** -0.5, tap.stats)
    aff = SelfAffinity(eng.sums, (h, w), eng.slices, eng.calls)
    tok = fd.FakeTokenizer()
    maps = np.zeros((13, h, w), np.float32)
    for i in compute_token_merge_indices(tok, PROMPT, 'bicycle', None)[0]:
        maps[i] = plane
    ghm = GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps).to(DEV))
    out = ghm.propagate(aff, iterations=2)

    class _Image:
        size = (w, h)
    before = JA.iou(ghm.segment(['bicycle'], _Image(), threshold=0.5).masks[0].cpu().numpy(), truth)
    after = JA.iou(out.segment(['bicycle'], _Image(), threshold=0.5).masks[0].cpu().numpy(), truth)
    calls = [(qk, kt, qk, float(np.float32(64 ** -0.5)), 1.0)]
    ref = JA.propagate64(JA.reference_sums(calls), plane.reshape(1, -1), 2)[0].reshape(h, w)
    ref = (ref - ref.min()) / (ref.max() - ref.min())
    want = JA.iou(ref > 0.5, truth)
    print(f'\nblock case 12 x 20: IoU {before:.3f} -> {after:.3f}, float64 path {want:.3f}')
    assert after > before and after == want
