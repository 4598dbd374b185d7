"""Non-square generations on the device: ``finalize_rect_kernel`` (planes [h, w] -> maps [out_h, out_w]) through the raw C ABI, the tap
routes on layers whose ``hw`` is not a square, the orientation of every view, and a traced generation with ``height=`` / ``width=``.

Finalize reference (``tests/_rect_domain.py``, which ``tests/test_gpu_rect_domain.py`` uses on multi-key walks): float64 numpy,
``oracle.heatmap_oracle.bicubic_taps`` (torch's f32 coefficients) applied along the rows and then down the columns, clamp at 0, mean over
the keys.  With equal sides it is held against the oracle's ``global_heat_map``
(``test_reference_agrees_with_the_oracle_on_squares``).  Bound: the accuracy class include/daam_hip.h documents for f32 arithmetic on
any finite planes, per token row t: max |out - exact| <= 2^-19 * max |exact|.
Tap reference: the oracle's ``attention_probs``, kept half, reshaped [h, w] row-major; tolerances of
``test_gpu_parity.py::test_tap_qk_vs_oracle`` for the same dtype mode; and, per probability, the float64 softmax at the bound of
``tests/_tap_domain.py`` (``test_taps_on_rectangular_layers_per_probability``)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _attend_domain as ad
import _rect_domain as rd
import _tap_domain as td
from oracle import fake_diffusers as fd
from oracle import heatmap_oracle as ho
from test_gpu_layouts import _configure
from test_gpu_parity import _dev, _qk, _to_bh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOKENS = 77
NP_DT = {'f16': np.float16, 'bf16': ho.BF16, 'f32': np.float32}
TORCH_DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
CODE = {'f16': 0, 'f32': 1, 'bf16': 2}


def _nat():
    from daam_amd import _native as nat
    return nat, nat.load()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _kernels(nat, lib, ctx, which):
    buf = ctypes.create_string_buffer(256)
    nat.check(lib.daam_last_kernels(ctx, which, buf, len(buf)))
    return buf.value.decode()


# ---- the float64 reference: tests/_rect_domain.py ----------------------------------------------------------------------------------
_resize64, _global64 = rd.resize64, rd.global64


def _assert_rows(got, want, what):
    """err_t <= 2^-19 * rowmax_t for every token row (printed before it is asserted)."""
    got = got.astype(np.float64)
    err = np.abs(got - want).reshape(want.shape[0], -1).max(1)
    rowmax = np.abs(want).reshape(want.shape[0], -1).max(1)
    worst = (err / np.maximum(rowmax, 1e-300)).max()
    print(f'{what}: worst err_t / rowmax_t = 2^{np.log2(max(worst, 1e-300)):.1f}')
    assert (err <= 2.0 ** -19 * rowmax).all(), f'{what}: 2^{np.log2(worst):.1f} of the row maximum'


def test_reference_agrees_with_the_oracle_on_squares():
    rng = np.random.default_rng(0)
    raw = [((f, layer, 0), (rng.standard_normal((TOKENS, s, s)) * 3).astype(np.float32))
           for layer, (f, s) in enumerate([(1, 64), (2, 32), (4, 16)])]
    want = ho.global_heat_map(raw, 4096, dtype=np.float32).astype(np.float64)
    mine = _global64([p for _, p in raw], 64, 64)
    err = np.abs(mine - want).reshape(TOKENS, -1).max(1)
    assert (err <= 2.0 ** -19 * np.abs(want).reshape(TOKENS, -1).max(1)).all()       # the oracle's own f32 arithmetic


# ---- finalize --------------------------------------------------------------------------------------------------------------------
class _Ctx:
    """A context made through the rect entry points, its layers' sums in torch buffers of ours."""

    def __init__(self, out_hw, layers, dt, heads=2, seed=0, square_api=False):
        self.nat, self.lib = _nat()
        self.out_hw, self.dt, self.heads = out_hw, dt, heads
        self.ctx = self.nat.c_void_p()
        if square_api:
            self.nat.check(self.lib.daam_ctx_create(len(layers), TOKENS, out_hw[0], CODE[dt], self.nat.byref(self.ctx)))
        else:
            self.nat.check(self.lib.daam_ctx_create_rect(len(layers), TOKENS, out_hw[0], out_hw[1], CODE[dt], self.nat.byref(self.ctx)))
        rng = np.random.default_rng(seed)
        self.bufs, self.planes = [], []          # planes: [layer][head] -> [77, h, w] as the device holds them (float32 values)
        for i, (h, w) in enumerate(layers):
            x = (rng.standard_normal((heads, TOKENS, h, w)) * 3).astype(np.float32)      # signed: the clamp matters
            x = ho.round_bf16(x) if dt == 'bf16' else x.astype(NP_DT[dt]).astype(np.float32)
            buf = torch.from_numpy(x).to(DEV).to(TORCH_DT[dt]).contiguous()
            if square_api:
                self.nat.check(self.lib.daam_layer_configure(self.ctx, i, heads, h, out_hw[0] // h, buf.data_ptr()))
            else:
                self.nat.check(self.lib.daam_layer_configure_rect(self.ctx, i, heads, h, w, max(1, out_hw[0] // h), buf.data_ptr()))
            self.bufs.append(buf)
            self.planes.append(x)

    def keys(self, mask=None):
        flat = [self.planes[i][h] for i in range(len(self.planes)) for h in range(self.heads)]
        return [p for j, p in enumerate(flat) if mask is None or mask[j]]

    def finalize(self, mask=None, n_rows=0, out=None):
        oh, ow = self.out_hw
        if out is None:
            out = torch.empty(TOKENS if n_rows <= 0 else n_rows, oh, ow, dtype=torch.float32, device=DEV)
        m = None if mask is None else (ctypes.c_uint8 * len(mask))(*mask)
        self.nat.check(self.lib.daam_finalize(self.ctx, m, n_rows, out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        return out

    def close(self):
        self.lib.daam_ctx_destroy(self.ctx)


FIN_CASES = [
    ((12, 20), [(12, 20), (6, 10), (3, 5)]),           # the output's size, x2, x4; 60 and 15 elements: no 16-byte pieces
    ((52, 76), [(52, 76), (26, 38)]),                  # SDXL at 832 x 1216
    ((64, 128), [(32, 64)]),                           # the widest output
]


@pytest.mark.parametrize('dt', ['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('out_hw,layers', FIN_CASES)
def test_finalize_rect(out_hw, layers, dt):
    c = _Ctx(out_hw, layers, dt, seed=out_hw[0])
    try:
        oh, ow = out_hw
        n_keys = len(layers) * c.heads
        want = _global64(c.keys(), oh, ow)
        got = c.finalize()
        assert _kernels(c.nat, c.lib, c.ctx, 1) == 'finalize_rect_kernel<%s>' % dt
        _assert_rows(got.cpu().numpy(), want, f'{out_hw} {dt} all keys')
        # a key-mask subset
        mask = [1 if j % 3 != 1 else 0 for j in range(n_keys)]
        _assert_rows(c.finalize(mask).cpu().numpy(), _global64(c.keys(mask), oh, ow), f'{out_hw} {dt} mask')
        # n_rows = 5: the rows beyond are neither read nor written
        buf = torch.full((TOKENS, oh, ow), -123.0, dtype=torch.float32, device=DEV)
        c.finalize(n_rows=5, out=buf)
        _assert_rows(buf[:5].cpu().numpy(), want[:5], f'{out_hw} {dt} n_rows=5')
        assert bool((buf[5:] == -123.0).all())
        # two groups with different row counts
        kg = [j % 2 for j in range(n_keys)]
        rows = [7, TOKENS]
        out = torch.full((2, TOKENS, oh, ow), -123.0, dtype=torch.float32, device=DEV)
        i32 = ctypes.c_int32
        c.nat.check(c.lib.daam_finalize_groups(c.ctx, (i32 * n_keys)(*kg), 2, (i32 * 2)(*rows), out.data_ptr(), TOKENS * oh * ow, _stream()))
        torch.cuda.synchronize()
        assert _kernels(c.nat, c.lib, c.ctx, 1) == 'finalize_rect_grouped_kernel<%s>' % dt
        for g in range(2):
            want_g = _global64(c.keys([int(k == g) for k in kg]), oh, ow)
            _assert_rows(out[g, :rows[g]].cpu().numpy(), want_g[:rows[g]], f'{out_hw} {dt} group {g}')
        assert bool((out[0, 7:] == -123.0).all())
    finally:
        c.close()


def test_rect_context_exclusions():
    """What a context of unequal sides does not offer is refused, not guessed: time windows, the announced finalize; and a selection
    whose planes need more LDS than a workgroup has is DAAM_E_UNSUPPORTED, never launched."""
    c = _Ctx((12, 20), [(6, 10)], 'f16')
    try:
        i32 = ctypes.c_int32
        assert c.lib.daam_ctx_set_time_bins(c.ctx, 2, (i32 * 2)(0, 3)) == c.nat.E_UNSUPPORTED
        out = torch.zeros(TOKENS, 12, 20, dtype=torch.float32, device=DEV)
        assert c.lib.daam_finalize_prepare(c.ctx, None, 0, out.data_ptr(), _stream()) == c.nat.E_UNSUPPORTED
        # two groups over the same keys of the one window: the window-range reduction, which such a context does not have
        out2 = torch.zeros(2, TOKENS, 12, 20, dtype=torch.float32, device=DEV)
        rc = c.lib.daam_finalize_bins(c.ctx, (i32 * 2)(0, 0), 2, (i32 * 2)(0, 0), (i32 * 2)(0, 0), (i32 * 2)(1, 1), (i32 * 2)(5, 5),
                                      out2.data_ptr(), TOKENS * 12 * 20, _stream())
        assert rc == c.nat.E_UNSUPPORTED
        c.finalize(n_rows=3)                                       # the context still serves a plain finalize afterwards
    finally:
        c.close()
    big = _Ctx((128, 64), [(128, 96)], 'f32', heads=1)           # 8192 + 12288 + 8192 floats = 112 KB of LDS: above the 64 KB default, fits
    try:
        got = big.finalize(n_rows=1)
        _assert_rows(got.cpu().numpy(), _global64(big.keys(), 128, 64)[:1], '(128, 64) f32 with 112 KB of LDS')
    finally:
        big.close()
    too_big = _Ctx((128, 128), [(128, 96)], 'f32', heads=1)      # 16384 + 12288 + 16384 floats = 176 KB > 160 KB
    try:
        out = torch.zeros(1, 128, 128, dtype=torch.float32, device=DEV)
        assert too_big.lib.daam_finalize(too_big.ctx, None, 1, out.data_ptr(), _stream()) == too_big.nat.E_UNSUPPORTED
    finally:
        too_big.close()


def test_nothing_moved_for_squares():
    """A square context made through the _rect entry points is the context daam_ctx_create makes: same kernels, same bits."""
    res = []
    for square_api in (True, False):
        c = _Ctx((64, 64), [(32, 32), (64, 64)], 'f16', heads=3, seed=5, square_api=square_api)
        try:
            out = c.finalize(n_rows=9)
            res.append((out.cpu(), _kernels(c.nat, c.lib, c.ctx, 1)))
        finally:
            c.close()
    assert res[0][1] == res[1][1] and 'rect' not in res[0][1] and 'finalize_up32_pipe_kernel' in res[0][1]
    assert torch.equal(res[0][0], res[1][0])


# ---- taps on rectangular layers ----------------------------------------------------------------------------------------------------
def _want_sums(qs, ks, heads, scale, np_dt, acc_np, h, w):
    """The oracle's running sums of the kept half, [kept, 77, h, w] (row-major pixels), float64."""
    raw = ho.RawMaps(acc_np)
    for q, k in zip(qs, ks):
        probs = ho.attention_probs(_to_bh(q, heads), _to_bh(k, heads), scale, np_dt)
        kept = probs[probs.shape[0] // 2:]
        maps = np.ascontiguousarray(kept.transpose(0, 2, 1)).reshape(kept.shape[0], TOKENS, h, w)
        for head in range(maps.shape[0]):
            raw.update(1, 0, head, maps[head])
    return np.stack([v for _, v in raw]).astype(np.float64)


def _tol(mode, steps, want):
    half_ulp = 2.0 ** -8 if mode == 'bf16' else 2.0 ** -11
    if mode == 'f32':
        return 2e-6 * max(1.0, np.abs(want).max())
    return 2 * half_ulp * max(1.0, want.max())               # 'exact' sums: 1 ulp of the largest running sum


@pytest.mark.parametrize('mode', ['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('d', [64, 40])
@pytest.mark.parametrize('hw_shape', [(6, 10), (26, 38), (8, 24)])
def test_taps_on_rectangular_layers(hw_shape, d, mode):
    nat, lib = _nat()
    h, w = hw_shape
    hw = h * w
    heads = 2 if d == 64 else 8
    batch, steps = 2, 3
    c = heads * d
    scale = d ** -0.5
    np_dt = NP_DT[mode]
    rng = np.random.default_rng(hw + d)
    qs, ks = zip(*[_qk(rng, batch, heads, hw, d, np_dt) for _ in range(steps)])
    tq = [_dev(q, np_dt) for q in qs]
    tk = [_dev(k, np_dt) for k in ks]
    kept = heads                                                   # batch 2: the conditional half
    ctx = nat.c_void_p()
    nat.check(lib.daam_ctx_create_rect(4, TOKENS, 2 * h, 2 * w, CODE[mode], nat.byref(ctx)))
    bufs = [torch.zeros(kept, TOKENS, h, w, dtype=TORCH_DT[mode], device=DEV) for _ in range(4)]
    try:
        for layer in range(4):
            nat.check(lib.daam_layer_configure_rect(ctx, layer, kept, h, w, 2, bufs[layer].data_ptr()))
        desc = nat.QKDesc(in_dtype=CODE[mode], batch=batch, heads=heads, hw=hw, tokens=TOKENS, head_dim=d, round_logits=1, scale=scale,
                          q_stride_b=hw * c, q_stride_h=d, q_stride_p=c, k_stride_b=TOKENS * c, k_stride_h=d, k_stride_t=c)
        s = _stream()
        # a call whose hw is not the layer's h * w is refused
        bad = nat.QKDesc.from_buffer_copy(bytes(desc))
        bad.hw = hw - 1
        assert lib.daam_tap_qk(ctx, 0, tq[0].data_ptr(), tk[0].data_ptr(), nat.byref(bad), s) == nat.E_INVALID
        # route 1: immediate taps
        for q, k in zip(tq, tk):
            nat.check(lib.daam_tap_qk(ctx, 0, q.data_ptr(), k.data_ptr(), nat.byref(desc), s))
        immediate = _kernels(nat, lib, ctx, 0)
        # route 2: three recorded steps, one launch
        for q, k in zip(tq, tk):
            nat.check(lib.daam_tap_qk_enqueue(ctx, 1, q.data_ptr(), k.data_ptr(), nat.byref(desc)))
        nat.check(lib.daam_tap_flush(ctx, s))
        deferred = _kernels(nat, lib, ctx, 0)
        # route 3: materialised probabilities
        for q, k in zip(qs, ks):
            probs = ho.attention_probs(_to_bh(q, heads), _to_bh(k, heads), scale, np_dt)
            p = _dev(probs, np_dt)
            nat.check(lib.daam_tap_probs(ctx, 2, p.data_ptr(), CODE[mode], batch * heads, hw, TOKENS, s))
        # route 4: the fused attention, where daam_attend_supported accepts
        v = [torch.randn_like(k) for k in tk]
        out = torch.empty_like(tq[0])
        adesc = nat.AttendDesc(qk=desc, v_stride_b=TOKENS * c, v_stride_h=d, v_stride_t=c, o_stride_b=hw * c, o_stride_h=d, o_stride_p=c)
        takes = lib.daam_attend_supported(nat.byref(adesc), tq[0].data_ptr(), tk[0].data_ptr(), v[0].data_ptr(), out.data_ptr())
        assert bool(takes) == (hw % 8 == 0 and mode != 'f32'), (hw, mode, takes)
        for q, k, vv in zip(tq, tk, v):
            rc = lib.daam_attend(ctx, 3, q.data_ptr(), k.data_ptr(), vv.data_ptr(), out.data_ptr(), nat.byref(adesc), 1, s)
            assert rc == (0 if takes else nat.E_UNSUPPORTED)
            if not takes:                                          # the caller's fallback: its own attention plus daam_tap_qk
                nat.check(lib.daam_tap_qk(ctx, 3, q.data_ptr(), k.data_ptr(), nat.byref(desc), s))
        torch.cuda.synchronize()
        if hw % 8:
            assert 'tap_generic_kernel' in immediate and 'tap_generic_kernel' in deferred, (immediate, deferred)
        want = _want_sums(qs, ks, heads, scale, np_dt, np_dt, h, w)
        tol = _tol(mode, steps, want)
        for layer, route in enumerate(('tap_qk', 'enqueue + flush', 'tap_probs', 'attend' if takes else 'attend declined + tap_qk')):
            got = bufs[layer].float().cpu().numpy().astype(np.float64)
            err = np.abs(got - want).max()
            print(f'{hw_shape} d={d} {mode} {route}: max-abs {err:.3e} (tol {tol:.3e})')
            if route == 'tap_probs':
                np.testing.assert_array_equal(got, want)          # the same adds in the same order
            else:
                assert err <= tol, f'{route}: {err} > {tol}'
        if not takes:                                              # the fallback IS the stand-alone tap: the same bits
            assert torch.equal(bufs[3], bufs[0])
    finally:
        lib.daam_ctx_destroy(ctx)


_tap_inputs, _tap_refs = {}, {}


def _tap_reference(hw, heads, d, np_dt, n_steps, acc_np):
    """``_attend_domain.build`` rows and ``_tap_domain.reference`` of them, computed once per shape, pipeline and sum dtype."""
    key = (hw, heads, d, str(np_dt), n_steps)
    if key not in _tap_inputs:
        _tap_inputs[key] = ad.build(hw, heads, d, np_dt, n_steps)
    steps, names = _tap_inputs[key]
    if key + (str(acc_np),) not in _tap_refs:
        _tap_refs[key + (str(acc_np),)] = td.reference(steps, heads, d ** -0.5, np_dt, acc_np)
    return steps, names, _tap_refs[key + (str(acc_np),)]


@pytest.mark.parametrize('mode,sums', [('f16', 'f16'), ('f16', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32'), ('f32', 'f32')])
@pytest.mark.parametrize('d', [64, 40])
@pytest.mark.parametrize('hw_shape', [(6, 10), (26, 38), (8, 24)])
def test_taps_on_rectangular_layers_per_probability(hw_shape, d, mode, sums, monkeypatch):
    """The routes of ``test_taps_on_rectangular_layers`` on the rows of ``tests/_attend_domain.py``, every sum element against the float64
    softmax at ``tests/_tap_domain.py``'s own bound (as ``tests/test_gpu_tap_domain.py::_run_route`` judges the square layers): 60 pixels are
    less than one 64-pixel wave tile, 988 end in a ragged one, 192 take the MFMA kernels.  ``sums``: the dtype of the running sums; f32
    sums under a 16-bit pipeline also carry the rounding-bias rule wherever the layer has the 4096 elements it asks for."""
    _configure(monkeypatch, {})                                    # no kernel switch left over from another test
    nat, lib = _nat()
    h, w = hw_shape
    hw = h * w
    heads = 2 if d == 64 else 8
    batch, steps_n = 2, 3
    c = heads * d
    np_dt, acc_np = NP_DT[mode], NP_DT[sums]
    steps, names, ref = _tap_reference(hw, heads, d, np_dt, steps_n, acc_np)
    tq = [_dev(q, np_dt) for q, _ in steps]
    tk = [_dev(k, np_dt) for _, k in steps]
    tv = [_dev(v, np_dt) for v in ad.values('plain', heads, d, np_dt, steps_n)]
    tp = [_dev(ho.attention_probs(_to_bh(q, heads), _to_bh(k, heads), d ** -0.5, np_dt), np_dt) for q, k in steps]
    inputs = tq + tk + tv + tp
    before = [t.clone() for t in inputs]
    generic = hw % 8 != 0 or mode == 'f32'
    want_name = ('tap_generic_kernel',) * 2 if generic else ('tap_d64_kernel', 'tap_slab_kernel' if (mode, d) == ('f16', 40) else 'tap_d64_kernel')
    ctx = nat.c_void_p()
    nat.check(lib.daam_ctx_create_rect(4, TOKENS, 2 * h, 2 * w, CODE[sums], nat.byref(ctx)))
    bufs = [torch.zeros(heads, TOKENS, h, w, dtype=TORCH_DT[sums], device=DEV) for _ in range(4)]
    try:
        for layer in range(4):
            nat.check(lib.daam_layer_configure_rect(ctx, layer, heads, h, w, 2, bufs[layer].data_ptr()))
        desc = nat.QKDesc(in_dtype=CODE[mode], batch=batch, heads=heads, hw=hw, tokens=TOKENS, head_dim=d, round_logits=1, scale=d ** -0.5,
                          q_stride_b=hw * c, q_stride_h=d, q_stride_p=c, k_stride_b=TOKENS * c, k_stride_h=d, k_stride_t=c)
        s = _stream()
        for q, k in zip(tq, tk):
            nat.check(lib.daam_tap_qk(ctx, 0, q.data_ptr(), k.data_ptr(), nat.byref(desc), s))
        assert _kernels(nat, lib, ctx, 0) == want_name[0], _kernels(nat, lib, ctx, 0)
        for q, k in zip(tq, tk):
            nat.check(lib.daam_tap_qk_enqueue(ctx, 1, q.data_ptr(), k.data_ptr(), nat.byref(desc)))
        nat.check(lib.daam_tap_flush(ctx, s))
        assert _kernels(nat, lib, ctx, 0) == want_name[1], _kernels(nat, lib, ctx, 0)
        for p in tp:
            nat.check(lib.daam_tap_probs(ctx, 2, p.data_ptr(), CODE[mode], batch * heads, hw, TOKENS, s))
        out = torch.empty_like(tq[0])
        adesc = nat.AttendDesc(qk=desc, v_stride_b=TOKENS * c, v_stride_h=d, v_stride_t=c, o_stride_b=hw * c, o_stride_h=d, o_stride_p=c)
        takes = bool(lib.daam_attend_supported(nat.byref(adesc), tq[0].data_ptr(), tk[0].data_ptr(), tv[0].data_ptr(), out.data_ptr()))
        assert takes == (not generic), (hw, mode, takes)
        for q, k, v in zip(tq, tk, tv):
            if takes:
                nat.check(lib.daam_attend(ctx, 3, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), nat.byref(adesc), 1, s))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(inputs, before)), 'an input was written to'
        for layer, route in enumerate(('tap_qk', 'enqueue + flush', 'tap_probs', 'attend')[:4 if takes else 3]):
            what = f'{hw_shape} d={d} {mode} pipeline, {sums} sums, {route}'
            got = bufs[layer].float().cpu().numpy().astype(np.float64).reshape(heads, TOKENS, hw)
            td.assert_inside_bound(got, ref, names, what)
            if mode != 'f32' and sums == 'f32':
                if td.bias(got, ref, names, np_dt)[1] >= td.BIAS_MIN_COUNT:      # a count of the inputs: 60 pixels x 2 heads have too few
                    td.assert_unbiased(got, ref, names, np_dt, what)
                else:
                    assert (hw, heads) == (60, 2), (hw, heads)
    finally:
        lib.daam_ctx_destroy(ctx)


# ---- normalise, word maps and expand_as on maps of unequal sides ---------------------------------------------------------------------
def _assert_normalized(got, maps):
    """trace.py:129-130 on the device's own un-normalised ``maps`` [rows, h, w], at the bound of the square call
    (``test_gpu_parity.py::test_normalize_and_word_maps``)."""
    m = maps.cpu().numpy()
    want = m / (m[1:-1].sum(0, keepdims=True) + np.float32(1e-6))
    assert tuple(got.shape) == m.shape
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-6, atol=1e-7)


def _expand64(word, out_h, out_w, absolute=False, threshold=None):
    """heatmap.py:77-87 on a [h, w] word map in float64: bicubic, min-max unless ``absolute``, optional threshold."""
    v = _resize64(word, out_h, out_w)
    if not absolute:
        v = (v - v.min()) / (v.max() - v.min() + 1e-8)
    if threshold:
        v = (v > threshold).astype(np.float64)
    return v


def _assert_expanded(got, want, kw, what):
    """Tolerances of the square kernel (``test_gpu_parity.py::test_normalize_and_word_maps``)."""
    assert got.shape == want.shape, what
    if kw.get('threshold'):
        assert (got != want).mean() < 1e-4, what                  # values within 1e-6 of the threshold may flip
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5, err_msg=what)


@pytest.mark.parametrize('hw', [(12, 20), (52, 76), (7, 3)])
def test_rect_normalize_word_and_expand_values(hw):
    """``daam_epilogue_normalize_rect`` and ``daam_word_heat_map_rect`` (mean of several planes; resize from a source of unequal sides,
    to a larger, a smaller, an odd and the same size; absolute, min-max and threshold) against numpy.  The source's two sides differ and
    so do the two scale factors: swapped axes, weights or strides fail here."""
    from daam_amd import engine as E
    h, w = hw
    rng = np.random.default_rng(h * w)
    maps = np.abs(rng.standard_normal((9, h, w))).astype(np.float32)
    eng = E.HeatMapEngine(1, out_hw=hw)
    try:
        t = torch.from_numpy(maps.copy()).to(DEV)
        eng._require_device(t)
        _assert_normalized(eng.normalize_(t), torch.from_numpy(maps))
    finally:
        eng.close()
    gm = torch.from_numpy(maps).to(DEV)
    for idxs in ([4], [2, 3, 5], [8, 0, 1, 7, 6]):
        wm = E.word_heat_map(gm, idxs)
        want = maps[idxs].astype(np.float64).mean(0)
        np.testing.assert_allclose(wm.cpu().numpy(), want, rtol=1e-6, atol=1e-7, err_msg=str(idxs))
    word = wm.cpu().numpy()
    for size in ((2 * h, 2 * w), (h, w), (3 * h + 1, 2 * w + 5), (max(2, h // 2), max(2, w // 3)), (w, h)):
        for kw in (dict(), dict(absolute=True), dict(threshold=0.4)):
            got = E.expand_word_map(wm, *size, **kw).cpu().numpy()
            _assert_expanded(got, _expand64(word, *size, **kw), kw, f'{hw} -> {size} {kw}')


# ---- orientation ---------------------------------------------------------------------------------------------------------------------
def test_orientation_of_every_view():
    """Token t's probability mass sits on pixel (y, x) = (4, 7) of a 6 x 10 layer (y != x, h != w): the [h, w] sum view, the 12 x 20 global
    map and expand_as on a 40 x 24 image (PIL size = (width, height)) all peak there."""
    from daam_amd.engine import HeatMapEngine, word_heat_map
    from daam_amd.heatmap import WordHeatMap
    h, w, y, x, t, d, heads = 6, 10, 4, 7, 5, 8, 1
    q = torch.zeros(2, h * w, heads * d, dtype=torch.float16, device=DEV)
    k = torch.zeros(2, TOKENS, heads * d, dtype=torch.float16, device=DEV)
    q[:, y * w + x, 0] = 8.0
    k[:, t, 0] = 8.0                                               # logit 64 * 8^-0.5 at (pixel, token), 0 everywhere else
    eng = HeatMapEngine(1, out_hw=(12, 20))
    try:
        f, lh, lw = 2, h, w
        eng.tap_qk(0, q, k, heads, d ** -0.5, factor=f)
        (key, view), = list(eng.items())
        assert key == (2, 0, 0) and tuple(view.shape) == (TOKENS, h, w)
        assert divmod(int(view[t].float().argmax()), w) == (y, x)
        maps = eng.global_heat_map()
        assert tuple(maps.shape) == (TOKENS, 12, 20)
        gy, gx = divmod(int(maps[t].argmax()), 20)
        assert gy in (2 * y, 2 * y + 1) and gx in (2 * x, 2 * x + 1), (gy, gx)
        word = word_heat_map(maps, [t])
        assert tuple(word.shape) == (12, 20)
        try:
            from PIL import Image
            image = Image.new('RGB', (40, 24))
        except ImportError:
            image = types.SimpleNamespace(size=(40, 24))
        big = WordHeatMap(word).expand_as(image)
        assert tuple(big.shape) == (24, 40)                        # [image height, image width]
        by, bx = divmod(int(big.argmax()), 40)
        assert 4 * y <= by < 4 * y + 4 and 4 * x <= bx < 4 * x + 4, (by, bx)
        norm = eng.normalize_(maps[:8].clone())
        _assert_normalized(norm, maps[:8])
    finally:
        eng.close()


# ---- a traced generation ---------------------------------------------------------------------------------------------------------------
OUT_H, OUT_W, STEPS = 12, 20, 3


class _Crop(torch.nn.Module):
    def __init__(self, width):
        super().__init__()
        self.width = width

    def forward(self, e):
        return e[..., :self.width].contiguous()


def _rect_pipe(batch):
    """The SDXL-like stand-in on a 24 x 40 latent (192 x 320 px): its attn2 layers see 12 x 20 and 6 x 10 positions."""
    pipe = fd.make_pipe('sdxl', device=DEV, dtype=torch.float16, batch=batch, seed=7, mini=True, identity_proj=True, dim_head=64,
                        heads_scale=0.2, tblocks_cap=1, latent_size=24)
    width = 0
    for spec in pipe.unet.execution_order():
        spec.module.norm_cross = _Crop(spec.module.to_v.in_features)
        width = max(width, spec.module.to_v.in_features)

    def hidden(i, spec, step):
        g = pipe._gen(1, i, step)
        x = torch.randn(pipe.batch, spec.res * (spec.res * 5 // 3), spec.query_dim, generator=g)
        return x.to(pipe.dtype).to(pipe.device)

    def context(i, spec):
        g = pipe._gen(2, i)
        ctx = torch.randn(pipe.batch, TOKENS, width, generator=g)
        ctx[:, 0, :] *= pipe.sos_gain
        return ctx.to(pipe.dtype).to(pipe.device)
    pipe.hidden_states, pipe.context = hidden, context
    return pipe, width


def _replay(pipe, key_of=None):
    """The oracle's fp16 running sums of the generation: per layer [kept, 77, h, w]; ``key_of(i, spec)`` replaces the context."""
    sums = []
    hooked = {id(m) for m in ho.locate(pipe.unet)[0]}             # the trace's layers: not the mid block
    for i, spec in enumerate(pipe.unet.execution_order()):
        a = spec.module
        if id(a) not in hooked:
            continue
        h, w = spec.res, spec.res * 5 // 3
        raw = ho.RawMaps(np.float16)
        for step in range(STEPS):
            q = pipe.hidden_states(i, spec, step).cpu().numpy()
            ctx = pipe.context(i, spec) if key_of is None else key_of(i, spec)
            k = a.norm_cross(ctx).cpu().numpy()
            probs = ho.attention_probs(_to_bh(q, a.heads), _to_bh(k, a.heads), a.scale, np.float16)
            kept = probs[probs.shape[0] // 2:]
            maps = np.ascontiguousarray(kept.transpose(0, 2, 1)).reshape(kept.shape[0], TOKENS, h, w)
            for head in range(maps.shape[0]):
                raw.update(1, 0, head, maps[head])
        sums.append(np.stack([v for _, v in raw]).astype(np.float32))
    return sums


def _check_map(got, keys, what):
    """fp16 pipeline with fp16 sums against the literal fp16 reference: global heat maps <= 1e-3 max-abs (test_gpu_parity.py)."""
    want = _global64(keys, OUT_H, OUT_W)[:got.shape[0]]
    assert tuple(got.shape[1:]) == (OUT_H, OUT_W)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f'{what}: max-abs {err:.3e}')
    assert err <= 1e-3, f'{what}: {err}'


def test_traced_rectangular_generation():
    import daam_amd
    pipe, width = _rect_pipe(batch=2)
    g = torch.Generator(device='cpu').manual_seed(3)
    emb = torch.randn(1, TOKENS, width, generator=g)
    emb[:, 0] *= 3.0
    emb = emb.to(torch.float16).to(DEV)
    prompt = 'a cat and a dog'
    with daam_amd.trace(pipe, height=16 * OUT_H, width=16 * OUT_W, probes=['a cat'], probe_embeds=emb) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        hm = tc.compute_global_heat_map()
        assert 'finalize_rect_kernel' in tc.engine.last_kernels(1)
        sums = _replay(pipe)
        rows = len(pipe.tokenizer.tokenize(prompt)) + 2
        assert tuple(hm.heat_maps.shape) == (rows, OUT_H, OUT_W)
        _check_map(hm.heat_maps, [p for layer in sums for p in layer], 'global map')
        views = dict(tc.all_heat_maps)
        assert {tuple(v.shape[1:]) for v in views.values()} == {(12, 20), (6, 10)}
        assert {k[0] for k in views} == {1, 2}
        # filters and the normalised map
        f2 = tc.compute_global_heat_map(factors=[2])
        _check_map(f2.heat_maps, [p for layer in sums if layer.shape[-1] == 10 for p in layer], 'factors=[2]')
        nm = tc.compute_global_heat_map(normalize=True).heat_maps
        # the kernel on the device's own map, against numpy at the square call's bound; then the keyword, which runs the finalize
        # again: the n key chunks of an output element arrive as f32 atomics in any order, so two finalizes of the same non-negative
        # sums differ by at most 2 (n - 1) 2^-24 of the value, and so may numerator and denominator of the normalised map
        _assert_normalized(tc.engine.normalize_(hm.heat_maps.clone()), hm.heat_maps)
        m = hm.heat_maps.cpu().numpy()
        np.testing.assert_allclose(nm.cpu().numpy(), m / (m[1:-1].sum(0, keepdims=True) + np.float32(1e-6)),
                                   rtol=2e-6 + 4 * len(views) * 2.0 ** -24, atol=1e-7)
        # word maps: the mean of the word's rows, resized to [image height, image width]
        from daam_amd.utils import compute_token_merge_indices
        idxs, _ = compute_token_merge_indices(pipe.tokenizer, prompt, 'cat', None, 0)
        wm = hm.compute_word_heat_map('cat')
        word = hm.heat_maps.cpu().numpy()[list(idxs)].astype(np.float64).mean(0)
        np.testing.assert_allclose(wm.heatmap.cpu().numpy(), word, rtol=1e-6, atol=1e-7)
        image = types.SimpleNamespace(size=(320, 192))             # PIL: (width, height)
        for kw in (dict(absolute=True), dict()):
            big = wm.expand_as(image, **kw).numpy()
            _assert_expanded(big, _expand64(wm.heatmap.cpu().numpy(), 192, 320, **kw), kw, f'expand_as {kw}')
        # the probe: the same queries against the probe's keys
        pm = tc.compute_probe_heat_map(0)
        psums = _replay(pipe, key_of=lambda i, spec: emb.expand(pipe.batch, TOKENS, width))
        _check_map(pm.heat_maps, [p for layer in psums for p in layer], 'probe map')
    daam_amd.engine.release_parked_contexts()


def test_traced_rectangular_batch_of_two_prompts():
    import daam_amd
    pipe, _ = _rect_pipe(batch=4)                                  # [uncond x 2 ; cond x 2]
    prompts = ['a cat and a dog', 'green grass']
    with daam_amd.trace(pipe, height=16 * OUT_H, width=16 * OUT_W, batch_prompts=True) as tc:
        pipe(prompts, num_inference_steps=STEPS)
        maps = tc.compute_global_heat_maps()
        assert 'finalize_rect_grouped_kernel' in tc.engine.last_kernels(1)
        sums = _replay(pipe)
        for p, hm in enumerate(maps):
            keys = []
            for layer in sums:
                per = layer.shape[0] // 2                          # prompt p owns the block [p * kept / 2, (p + 1) * kept / 2)
                keys += list(layer[p * per:(p + 1) * per])
            assert hm.heat_maps.shape[0] == len(pipe.tokenizer.tokenize(prompts[p])) + 2
            _check_map(hm.heat_maps, keys, f'prompt {p}')
    daam_amd.engine.release_parked_contexts()
