"""``daam_self_affinity_accumulate`` / ``daam_self_affinity_propagate`` (include/daam_self_affinity.h) on the device,
through ctypes on guarded buffers and through the Python layer, held to the float64 reference of ``_self_affinity_domain`` inside the
bounds derived there: (a) every entry of ``sums``, absolutely; (b) the propagated maps against float64 fed the device's own sums;
(c) both combined against the pure float64 path.

A tile of sums is 128 x 128, a statistics block 128 rows, a key step 64: P = 1, 5, 63, 65 sit inside one tile on either side of
the key step, 130 and 257 give two and three tile edges in both directions with partial last tiles.  Figures of every case are printed
before they are asserted (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _self_affinity_domain as A
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64


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
    """``(uint16 memory image, (stride_b, stride_h, stride_p))`` of f32 [b, h, P, d] in the layout of to_q / to_k ('interleaved',
    [b, P, h d]) or packed [b, h, P, d]."""
    b, h, P, d = x.shape
    if layout == 'interleaved':
        return A.bits(x.transpose(0, 2, 1, 3), dtype), (P * h * d, d, h * d)
    return A.bits(x, dtype), (h * P * d, P * d, d)


def accumulate_raw(calls, dtype, layout):
    """The chain ``calls`` of ``(q, k, scale, weight)`` into one guarded ``sums`` pre-filled with NaN (the first call has
    ``accumulate == 0``), each with a workspace of exactly the bytes asked for: f32 [P, P], after checking every guard and that q and
    k are unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_self_affinity()
    b, h, P, d = calls[0][0].shape
    sums = _guarded(4 * P * P, 0xFF, 4)
    assert np.isnan(_get(sums, 4 * P * P, np.float32, (P, P))).all()
    for n, (q, k, scale, weight) in enumerate(calls):
        need = lib.daam_self_affinity_workspace(b, h, P)
        assert need >= 8 * b * h * P and need % 8 == 0
        (qm, qs), (km, ks) = _layout(q, dtype, layout), _layout(k, dtype, layout)
        bufs = dict(q=_guarded(qm.nbytes, 0), k=_guarded(km.nbytes, 0), ws=_guarded(need, 0x5A, 8))
        _put(bufs['q'], qm)
        _put(bufs['k'], km)
        before = {key: bufs[key][0].clone() for key in ('q', 'k')}
        ptr = lambda key: bufs[key][0].data_ptr() + bufs[key][1]
        nat.check_self_affinity(lib.daam_self_affinity_accumulate(
            ptr('q'), ptr('k'), A.DAAM_F16 if dtype == 'f16' else A.DAAM_BF16, b, h, P, d, *qs, *ks, scale, weight, int(n > 0),
            sums[0].data_ptr() + sums[1], ptr('ws'), need, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert _intact(bufs['q'], qm.nbytes) and _intact(bufs['k'], km.nbytes) and _intact(bufs['ws'], need) and _intact(sums, 4 * P * P)
        assert all(torch.equal(bufs[key][0], before[key]) for key in before), 'q or k changed'
    return _get(sums, 4 * P * P, np.float32, (P, P))


def propagate_raw(sums, maps, iterations):
    from daam_amd import _native as nat
    lib = nat.load_self_affinity()
    n, P = maps.shape
    need = lib.daam_self_affinity_propagate_workspace(n, P)
    assert need >= 4 * (n + 1) * P and need % 8 == 0
    sizes = dict(sums=4 * P * P, maps=4 * n * P, refined=4 * n * P, ws=need)
    offsets = dict(sums=4, maps=8, refined=12, ws=4)
    bufs = {key: _guarded(v, 0x5A if key == 'ws' else 0xFF, offsets[key]) for key, v in sizes.items()}
    _put(bufs['sums'], sums)
    _put(bufs['maps'], maps)
    before = {key: bufs[key][0].clone() for key in ('sums', 'maps')}
    ptr = lambda key: bufs[key][0].data_ptr() + bufs[key][1]
    nat.check_self_affinity(lib.daam_self_affinity_propagate(ptr('sums'), P, ptr('maps'), n, iterations, ptr('refined'), ptr('ws'), need,
                                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for key in bufs:
        assert _intact(bufs[key], sizes[key]), f'guard bytes around {key} changed'
    assert all(torch.equal(bufs[key][0], before[key]) for key in before), 'sums or maps changed'
    return _get(bufs['refined'], 4 * n * P, np.float32, (n, P))


# ---- accumulate ----------------------------------------------------------------------------------------------------------------------
PS = (1, 5, 63, 65, 130, 257)
SLICES = ((1, 1), (1, 3), (2, 3))                     # (batch, heads)
LAYOUTS = ('interleaved', 'packed')
# every P x head dim x dtype; the slice counts, layouts and regimes rotate so that each meets every P, every head dim and both dtypes
ACC_CASES = [(P, d, dtype, SLICES[(pi + di + ti) % 3], LAYOUTS[(pi + di // 2 + ti) % 2], A.REGIMES[(pi + di + 2 * ti) % 4])
             for pi, P in enumerate(PS) for di, d in enumerate(A.HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]


def _report(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f'\n{name}: worst error {err.max():.3e} bound there {float(bound.ravel()[(err / bound).argmax()]):.3e} worst device/bound {ratio:.3f}')
    return err, ratio


@pytest.mark.parametrize('P,d,dtype,slices,layout,regime', ACC_CASES,
                         ids=[f'P{c[0]}-d{c[1]}-{c[2]}-S{c[3][0]}x{c[3][1]}-{c[4]}-{c[5]}' for c in ACC_CASES])
def test_one_call_is_within_bound_a(P, d, dtype, slices, layout, regime):
    q, k, scale = A.inputs(regime, *slices, P, d, dtype, seed=P + d)
    calls = [(q, k, scale, 1.0)]
    got = accumulate_raw(calls, dtype, layout)
    assert np.array_equal(got.view(np.uint32), accumulate_raw(calls, dtype, layout).view(np.uint32)), 'a second run'
    want, bound = A.reference_sums(calls), A.sums_bound(calls)
    err, ratio = _report(f'accumulate P={P} d={d} {dtype} S={slices[0] * slices[1]} {layout} {regime}', got, want, bound)
    assert np.isfinite(got).all() and (err <= bound).all(), f'{ratio:.3f} of the bound'
    s = slices[0] * slices[1]
    assert np.abs(got.astype(np.float64).sum(axis=1) - s).max() <= bound.sum(axis=1).max() + P * A.U * s
    if regime == 'zero_q':
        assert np.abs(got - np.float32(s / P)).max() <= 4 * A.U * s / P * s


@pytest.mark.parametrize('P,d,dtype,layout', [(65, 64, 'f16', 'interleaved'), (130, 40, 'bf16', 'packed'), (257, 160, 'f16', 'interleaved')])
def test_two_calls_accumulate_and_a_negative_weight(P, d, dtype, layout):
    q1, k1, scale = A.inputs('small', 1, 3, P, d, dtype, seed=1)
    q2, k2, _ = A.inputs('outlier', 1, 3, P, d, dtype, seed=2)
    for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
        calls = [(q1, k1, scale, w1), (q2, k2, scale, w2)]
        got = accumulate_raw(calls, dtype, layout)
        want, bound = A.reference_sums(calls), A.sums_bound(calls)
        err, ratio = _report(f'two calls P={P} d={d} {dtype} weights {w1} {w2}', got, want, bound)
        assert (err <= bound).all(), f'{ratio:.3f} of the bound'


# ---- propagate -----------------------------------------------------------------------------------------------------------------------
def _synthetic_sums(P, seed=0):
    """f32 [P, P] >= 0: a banded structure plus noise, and (P > 1) one zero row."""
    rng = np.random.default_rng(seed + P)
    i = np.arange(P)
    s = np.exp(-np.abs(i[:, None] - i[None]) / max(P / 8, 1)) * rng.uniform(0.5, 1.5, (P, P))
    if P > 1:
        s[P // 3] = 0
    return s.astype(np.float32)


@pytest.mark.parametrize('P', (1, 5, 63, 65, 257, 1000))
@pytest.mark.parametrize('N', (1, 3, 32))
def test_propagate_is_within_bound_b(P, N):
    sums, m = _synthetic_sums(P), A.maps(N, P, seed=N, signed=True)
    for T in (0, 1, 2, 16):
        got = propagate_raw(sums, m, T)
        want, bound = A.reference_propagate(sums, m, T), A.propagate_bound(P, m, T)
        err = float(np.abs(got - want).max())
        print(f'\npropagate P={P} N={N} T={T}: worst error {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}')
        if T == 0:
            assert np.array_equal(got.view(np.uint32), m.view(np.uint32)), 'iterations = 0 returns the input bits'
        assert err <= bound
        assert got.min() >= m.min() - bound and got.max() <= m.max() + bound
        if P > 1:
            assert np.array_equal(got[:, P // 3], m[:, P // 3]), 'a zero row keeps its value'
    assert np.array_equal(propagate_raw(sums, m, 2), propagate_raw(sums, m, 2)), 'a second run'


@pytest.mark.parametrize('P', (5, 65, 257))
def test_identity_and_uniform_sums(P):
    m = A.maps(3, P, seed=3, signed=True)
    got = propagate_raw((4.0 * np.eye(P)).astype(np.float32), m, 3)
    assert np.array_equal(got, m), 'c I with c a power of two: every value is (4 m + zeros) / 4, exactly m'
    got = propagate_raw(np.full((P, P), 0.75, np.float32), m, 1)
    mean = m.astype(np.float64).mean(axis=1, keepdims=True)
    assert np.abs(got - mean).max() <= A.propagate_bound(P, m, 1)


@pytest.mark.parametrize('P,d,dtype', [(63, 40, 'f16'), (257, 64, 'bf16')])
def test_end_to_end_is_within_bound_c(P, d, dtype):
    q, k, scale = A.inputs('small', 1, 3, P, d, dtype, seed=9)
    calls = [(q, k, scale, 1.0)]
    sums = accumulate_raw(calls, dtype, 'interleaved')
    exact, delta = A.reference_sums(calls), A.sums_bound(calls)
    m = A.maps(3, P, seed=4)
    for T in (1, 2, 16):
        got = propagate_raw(sums, m, T)
        fed, pure = A.reference_propagate(sums, m, T), A.reference_propagate(exact, m, T)
        b, c = A.propagate_bound(P, m, T), A.combined_bound(delta, exact, m, T)
        eb, ec = float(np.abs(got - fed).max()), float(np.abs(got - pure).max())
        print(f'\nend to end P={P} T={T}: fed {eb:.3e} / {b:.3e} = {eb / b:.3f}; pure {ec:.3e} / {c:.3e} = {ec / c:.3f}')
        assert eb <= b and ec <= c


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def test_the_stand_in_unet_for_two_steps():
    """An 8 x 8 trace of a stand-in UNet with an ``attn1`` per transformer block: the affinity is the float64 sum over the tapped calls
    inside bound (a), the model's outputs are bit-equal to the untraced ones, and the counts are right."""
    import daam_amd
    from test_self_affinity_cpu import add_attn1, self_attention_calls
    steps = 2
    pipe = fd.make_pipe('sd15', device=DEV, dtype=torch.float16, batch=2, seed=3, mini=True, identity_proj=True, dim_head=40, latent_size=8)
    add_attn1(pipe)
    pipe.keep_outputs = True
    pipe(PROMPT, num_inference_steps=steps)
    plain = [o.clone() for o in pipe.last_outputs[0::2]]                  # the attn1 outputs
    with daam_amd.trace(pipe, height=64, width=64, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=steps)
        traced = [o.clone() for o in pipe.last_outputs[0::2]]
        aff = tc.compute_self_affinity()
    assert all(torch.equal(a, b) for a, b in zip(plain, traced))
    calls = self_attention_calls(pipe, steps, grid=64)
    assert aff.grid == (8, 8) and aff.calls == len(calls) and aff.slices == sum(c[0].shape[0] * c[0].shape[1] for c in calls) and calls
    want, bound = A.reference_sums(calls), A.sums_bound(calls)
    err, ratio = _report('stand-in UNet 8 x 8, two steps', aff.sums.cpu().numpy(), want, bound)
    assert (err <= bound).all()
    assert torch.allclose(aff.matrix().sum(dim=1), torch.ones(64, device=DEV), atol=1e-5)


def test_the_block_structured_case_through_global_heat_map_propagate():
    """Q = K = a two-valued feature per cell plus noise at 45 x 70: ``segment`` after ``propagate`` reaches the IoU the float64 path
    reaches."""
    from daam_amd import GlobalHeatMap, SelfAffinity, engine as E
    from daam_amd.utils import compute_token_merge_indices
    qk, truth, plane = A.block_case()
    h, w = A.BLOCK_GRID
    x = torch.from_numpy(qk[0].transpose(1, 0, 2).reshape(1, h * w, -1)).to(DEV, torch.float16)
    eng = E.SelfAffinityState(h, w)
    eng.tap(x, x, 1, 40 ** -0.5)
    aff = SelfAffinity(eng.sums, (h, w), eng.slices, eng.calls)
    tok = fd.FakeTokenizer()
    maps = np.zeros((13, h, w), np.float32)
    for i in compute_token_merge_indices(tok, PROMPT, 'bicycle', None)[0]:
        maps[i] = plane
    ghm = GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps).to(DEV))
    out = ghm.propagate(aff, iterations=2)
    assert isinstance(out, GlobalHeatMap) and out.heat_maps.shape == (13, h, w) and out.heat_maps.dtype == torch.float32

    class _Image:
        size = (w, h)
    before = A.iou(ghm.segment(['bicycle'], _Image(), threshold=0.5).masks[0].cpu().numpy(), truth)
    after = A.iou(out.segment(['bicycle'], _Image(), threshold=0.5).masks[0].cpu().numpy(), truth)
    calls = [(qk, qk, float(np.float32(40 ** -0.5)), 1.0)]
    ref = A.reference_propagate(A.reference_sums(calls), plane.reshape(1, -1), 2)[0].reshape(h, w)
    ref = (ref - ref.min()) / (ref.max() - ref.min())
    want = A.iou(ref > 0.5, truth)
    print(f'\nblock case 45 x 70: IoU {before:.3f} -> {after:.3f}, float64 path {want:.3f}')
    assert before < 0.7 and after >= want - 0.01 and after >= 0.95
    word = out.compute_word_heat_map('bicycle').heatmap.cpu().numpy().reshape(1, -1)
    sums = aff.sums.cpu().numpy()
    fed = A.reference_propagate(sums, plane.reshape(1, -1), 2)
    assert np.abs(word - fed).max() <= A.propagate_bound(h * w, plane, 2)
    with pytest.raises(ValueError, match='45 x 70.*9 x 14'):
        GlobalHeatMap(tok, PROMPT, torch.zeros(13, 9, 14, device=DEV)).propagate(aff)
