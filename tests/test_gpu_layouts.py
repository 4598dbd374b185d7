"""Strided Q / K / V / out layouts through the raw C ABI (include/daam_hip.h: ``DaamQKDesc`` / ``DaamAttendDesc`` strides): every
specialised tap kernel and ``daam_attend`` on layouts other than the contiguous ``[B, S, H*d]`` the engine passes.

Layouts (the logical data is the same in all of them; every step's tensors live in storages of their own):

  L0   contiguous ``[B, S, H*d]``: the baseline, the source of the expected bits
  L1   fused projection buffers: Q = columns [0, c) of ``[B, hw, 3c]``, K = columns [c, 2c) of ``[B, 77, 2c]`` (V = the other half
       of that buffer), out = columns [c, 2c) of ``[B, hw, 2c]``
  L2   head-major ``[B, H, S, d]`` (the reference's ``head_to_batch_dim``): stride_h = S*d, row stride d
  L3   padded and offset: row stride c + 8, batch stride S*(c + 8) + 8, the view starts 8 elements into its storage (a 16-byte
       aligned pointer that is not 32-byte aligned: no row starts on a cache line)
  L4a  row stride c + 4; L4b: the view starts 4 elements into its storage (8-byte aligned pointer) -- on ONE of the tensors.
       Outside every ``*_supported()`` predicate: the tap takes the any-shape kernel, ``daam_attend`` declines.

Everything of a strided storage that is not the logical tensor is NaN (inputs: one read of a wrong column makes a sum NaN) or a
sentinel (out).  L1-L3 must reproduce L0's sums BIT FOR BIT on the same kernel and block size (the same kernel does the same
arithmetic on the same numbers); the expected kernel names are written from the predicates in the sources (``_expected``).  L0 itself
is held against the numpy oracle with the tolerances of ``test_gpu_parity.py::test_tap_qk_vs_oracle``; L4 against L0 with the bound of
``test_raw_abi_strides_past_32_bit_offsets_fall_back`` ("another kernel").

Data: K's start-of-sequence row is scaled by 1.0 / 1.5 / 2.0 at steps 0 / 1 / 2, so a K tile of another step in a step's place moves
every sum far beyond an ulp, and the logits stay of the size (rarely past 4) at which a logit that the other kernel's summation order
moves across an fp16 rounding boundary (ulp <= 2^-9 below 4) changes a probability by p (1 - p) ulp < 2^-10: what the L4 bound assumes.
Shapes: batch 2, hw 576 (side 24: 2.25 eight-wave tiles, 4.5 four-wave tiles: partial-tile clamp and the waves outside run on the
strided rows) and hw 256 (exact tiles); three steps on the deferred routes (both K buffers reused, the fetch a step ahead crosses to
another step's pointer), two on the immediate ones (the second launch adds to sums that are there)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import heatmap_oracle as ho
from test_gpu_attend import _inputs as _attend_inputs, _reference_eager, _restated_f64
from test_gpu_parity import _dev, _engine, _oracle_steps, _qk

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BATCH = 2
OUT_SENTINEL = -7.0
SWITCHES = ('DAAM_TAP_SYNC', 'DAAM_TAP_W8', 'DAAM_STRICT_EXP', 'DAAM_TAP_SLAB', 'DAAM_TAP_WALK', 'DAAM_NO_D64', 'DAAM_TAP_CHUNKED',
            'DAAM_FORCE_GENERIC', 'DAAM_TAP_PAIR', 'DAAM_SLAB_TAIL')
LAYOUTS = ('L1', 'L2', 'L3')
L4 = ('L4a_q', 'L4a_k', 'L4b_q', 'L4b_k')
HWS = (576, 256)

# mode -> (numpy dtype of Q / K, torch dtype, accumulate, extra environment)
MODES = {
    'f16_exact': (np.float16, torch.float16, 'exact', {}),
    'f16_f32acc': (np.float16, torch.float16, 'float32', {}),
    'f16_strict': (np.float16, torch.float16, 'exact', dict(DAAM_STRICT_EXP='1')),
    'bf16_exact': (ho.BF16, torch.bfloat16, 'exact', {}),
    'bf16_f32acc': (ho.BF16, torch.bfloat16, 'float32', {}),
    'f32': (np.float32, torch.float32, 'exact', {}),
}

# route -> head_dim, heads (8 / 4 / 2 for 40 / 80 / 160: the slab predicate's head conditions), deferred launch or immediate calls,
# switches, time windows, the (kernel, block size) of a layout every predicate accepts, and the dtype modes
_D64 = ('f16_exact', 'bf16_exact', 'f16_f32acc')
ROUTES = {
    'd64_immediate': dict(d=64, heads=2, deferred=False, env={}, kernel=('tap_d64_kernel', 256), modes=_D64),
    'd64_deferred': dict(d=64, heads=2, deferred=True, env={}, kernel=('tap_d64_kernel', 512), modes=_D64 + ('f16_strict',)),
    'd64_deferred_sync0': dict(d=64, heads=2, deferred=True, env=dict(DAAM_TAP_SYNC='0'), kernel=('tap_d64_kernel', 512), modes=('f16_exact',)),
    'd64_deferred_w4': dict(d=64, heads=2, deferred=True, env=dict(DAAM_TAP_W8='0'), kernel=('tap_d64_kernel', 256), modes=('f16_exact',)),
    'd40_partial': dict(d=40, heads=8, deferred=False, env=dict(DAAM_TAP_SLAB='0'), kernel=('tap_d64_kernel', 256), modes=('f16_exact',)),
    'walk': dict(d=64, heads=2, deferred=True, env=dict(DAAM_TAP_WALK='1'), bins=[0, 1, 2], kernel=('tap_walk_kernel', 512),
                 modes=('f16_exact', 'bf16_f32acc')),
    'wide80': dict(d=80, heads=4, deferred=False, env={}, kernel=('tap_wide_kernel', 256), modes=('f16_exact',)),
    'wide160': dict(d=160, heads=2, deferred=False, env={}, kernel=('tap_wide_kernel', 256), modes=('f16_exact',)),
    'mfma': dict(d=64, heads=2, deferred=False, env=dict(DAAM_NO_D64='1'), kernel=('tap_mfma_kernel', 256), modes=('f16_exact',)),
    'chunk40': dict(d=40, heads=8, deferred=False, env=dict(DAAM_TAP_CHUNKED='1'), kernel=('tap_chunk_kernel', 256), modes=('f16_exact',)),
    'chunk80_bf16': dict(d=80, heads=4, deferred=False, env={}, kernel=('tap_chunk_kernel', 256), modes=('bf16_exact',)),
    'slab40': dict(d=40, heads=8, deferred=True, env={}, kernel=('tap_slab_kernel', 512), modes=('f16_exact', 'f16_f32acc')),
    'slab80': dict(d=80, heads=4, deferred=True, env={}, kernel=('tap_slab_kernel', 512), modes=('f16_exact', 'f16_f32acc')),
    'slab160': dict(d=160, heads=2, deferred=True, env={}, kernel=('tap_slab_kernel', 512), modes=('f16_exact', 'f16_f32acc')),
    'any_shape_f32': dict(d=64, heads=2, deferred=False, env={}, kernel=('tap_generic_kernel', 256), modes=('f32',)),
}
ROUTE_MODES = [(r, m) for r, spec in ROUTES.items() for m in spec['modes']]
ROUTE_F16 = [(r, m) for r, m in ROUTE_MODES if m.startswith('f16')]       # L4 is defined on fp16 pipelines


def _expected(route, layout):
    """(kernel name, block size) from the predicates in daam_amd/csrc (not from a run).  L1-L3 have strides that are non-negative
    multiples of 8 far below 2^30 and 16-byte aligned pointers, which is all tap_d64 / tap_wide / tap_mfma / tap_chunk_supported()
    and offsets_fit_32() ask of a layout.  tap_slab_supported() also wants the heads adjacent in a row (q_sh == k_sh == head_dim):
    L2 (stride_h = S*d) leaves the slab kernel, and the layer keeps the kind mfma_kind() gave it -- head_dim 40: tap_d64_kernel,
    not FULL64, hence four waves; 80 / 160: tap_wide_kernel.  L4: tap_mfma_supported() (strides % 8) resp. use_mfma() (pointer & 15)
    fail for fp16, and the bf16 predicates are tap_d64 / tap_chunk_supported() with the same two conditions: the any-shape kernel."""
    if layout.startswith('L4'):
        return 'tap_generic_kernel', 256
    if route.startswith('slab') and layout == 'L2':
        return ('tap_d64_kernel', 256) if ROUTES[route]['d'] == 40 else ('tap_wide_kernel', 256)
    return ROUTES[route]['kernel']


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def _spec(layout, role, rows, heads, d):
    """(storage elements, first element, stride_b, stride_h, row stride), in elements, of tensor ``role`` [BATCH, rows, heads*d]."""
    c = heads * d
    if layout == 'L1':
        width, col = {'q': (3 * c, 0), 'k': (2 * c, c), 'v': (2 * c, 0), 'out': (2 * c, c)}[role]
        return BATCH * rows * width, col, rows * width, d, width
    if layout == 'L2':
        return BATCH * heads * rows * d, 0, heads * rows * d, rows * d, d
    if layout == 'L3':
        sb = rows * (c + 8) + 8
        return 8 + BATCH * sb, 8, sb, d, c + 8
    if layout == 'L4a':
        return BATCH * rows * (c + 4), 0, rows * (c + 4), d, c + 4
    if layout == 'L4b':
        return BATCH * rows * c + 4, 4, rows * c, d, c
    assert layout == 'L0', layout
    return BATCH * rows * c, 0, rows * c, d, c


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Placed:
    """A logical [BATCH, rows, heads*d] tensor laid out in a storage of its own (or in ``storage``: the KV buffer of L1)."""

    def __init__(self, x, layout, role, heads, fill, storage=None):
        b, rows, c = x.shape
        assert b == BATCH
        d = c // heads
        n, first, sb, sh, sp = _spec(layout, role, rows, heads, d)
        self.storage = torch.full((n,), fill, dtype=x.dtype, device=DEV) if storage is None else storage
        assert self.storage.numel() == n and self.storage.data_ptr() % 128 == 0
        self.view = torch.as_strided(self.storage, (b, rows, heads, d), (sb, sp, sh, 1), first)
        self.view.copy_(x.reshape(b, rows, heads, d))
        self.gaps = torch.ones(n, dtype=torch.bool, device=DEV)
        torch.as_strided(self.gaps, (b, rows, heads, d), (sb, sp, sh, 1), first).fill_(False)
        self.ptr = self.storage.data_ptr() + first * x.element_size()
        self.strides = (sb, sh, sp)
        self.shape = (b, rows, c)
        if layout == 'L3' and x.element_size() == 2:
            assert self.ptr % 32 == 16                        # 16-byte aligned, on no 32- / 64- / 128-byte boundary
        self.before = self.storage.clone()

    def unchanged(self):
        return torch.equal(_bits(self.storage), _bits(self.before))

    def logical(self):
        return self.view.reshape(self.shape).clone()


def _layout_of(layout, role):
    """'L4a_k' puts K alone into L4a; the other tensors of the call stay contiguous."""
    if not layout.startswith('L4'):
        return layout
    kind, who = layout.split('_')
    return kind if who == role else 'L0'


def _configure(monkeypatch, env):
    from daam_amd import engine as E
    E.release_parked_contexts()                               # the switches are read when a native context is created
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)


def _qk_desc(nat, dtype, heads, hw, d, q, k, round_logits=1):
    code = {torch.float16: 0, torch.float32: 1, torch.bfloat16: 2}[dtype]
    return nat.QKDesc(in_dtype=code, batch=BATCH, heads=heads, hw=hw, tokens=77, head_dim=d, round_logits=round_logits, scale=float(d ** -0.5),
                      q_stride_b=q.strides[0], q_stride_h=q.strides[1], q_stride_p=q.strides[2],
                      k_stride_b=k.strides[0], k_stride_h=k.strides[1], k_stride_t=k.strides[2])


def _raw_engine(dtype, accumulate, heads, hw, bins=None):
    eng = _engine(n_layers=1, accumulate=accumulate, defer_steps=0, time_bins=bins)
    eng._require_device(torch.empty(1, device=DEV))           # binds the engine to the device (tap_qk does this)
    eng._ensure_ctx(dtype)
    eng._ensure_layer(0, BATCH * heads - (BATCH * heads) // 2, int(math.isqrt(hw)), 1)
    eng._touch(0)
    return eng


def _last_launch(nat, eng):
    grid, block, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nat.check(eng.lib.daam_last_launch(eng.ctx, 0, ctypes.byref(grid), ctypes.byref(block), ctypes.byref(lds)))
    return eng.last_kernels(0), block.value


def _tap_raw(steps, heads, d, hw, dtype, accumulate, layout, deferred, bins=None, round_logits=1):
    """Tap ``steps`` = [(q, k)] (logical device tensors) through the C ABI with Q / K laid out in ``layout``.  Returns the sums
    (a binned context: [windows, heads, 77, side, side]), the kernel name and block size of the last launch, and whether every
    input storage is bit-unchanged."""
    from daam_amd import _native as nat
    eng = _raw_engine(dtype, accumulate, heads, hw, bins)
    placed = [(_Placed(q, _layout_of(layout, 'q'), 'q', heads, float('nan')), _Placed(k, _layout_of(layout, 'k'), 'k', heads, float('nan')))
              for q, k in steps]
    desc = _qk_desc(nat, dtype, heads, hw, d, *placed[0], round_logits=round_logits)
    for q, k in placed:
        if deferred:
            nat.check(eng.lib.daam_tap_qk_enqueue(eng.ctx, 0, q.ptr, k.ptr, ctypes.byref(desc)))
        else:
            nat.check(eng.lib.daam_tap_qk(eng.ctx, 0, q.ptr, k.ptr, ctypes.byref(desc), eng.stream))
    if deferred:
        nat.check(eng.lib.daam_tap_flush(eng.ctx, eng.stream))
    torch.cuda.synchronize()
    name, block = _last_launch(nat, eng)
    sums = eng.acc[0].clone().cpu()
    intact = all(q.unchanged() and k.unchanged() for q, k in placed)
    eng.close()
    return dict(sums=sums, name=name, block=block, intact=intact)


_data_cache, _run_cache, _oracle_cache = {}, {}, {}


def _data(hw, heads, d, np_dt):
    key = (hw, heads, d, str(np_dt))
    if key not in _data_cache:
        rng = np.random.default_rng(hw + 7 * d + heads + len(key[3]))
        _data_cache[key] = [_qk(rng, BATCH, heads, hw, d, np_dt, sos_gain=1.0 + 0.5 * s) for s in range(3)]
    return _data_cache[key]


def _n_steps(route):
    return 3 if ROUTES[route]['deferred'] else 2


def _run(monkeypatch, route, mode, hw, layout):
    key = (route, mode, hw, layout)
    if key not in _run_cache:
        r = ROUTES[route]
        np_dt, dtype, accumulate, env = MODES[mode]
        _configure(monkeypatch, dict(r['env'], **env))
        steps = [(_dev(q, np_dt), _dev(k, np_dt)) for q, k in _data(hw, r['heads'], r['d'], np_dt)[:_n_steps(route)]]
        _run_cache[key] = _tap_raw(steps, r['heads'], r['d'], hw, dtype, accumulate, layout, r['deferred'], r.get('bins'))
    return _run_cache[key]


def _check_sane(res, route, mode, what):
    """No NaN, not all zero, inputs untouched, and every step's probabilities sum to one over the tokens."""
    sums = res['sums'].float()
    assert res['intact'], f'{what}: an input storage was written to'
    assert not torch.isnan(sums).any(), f'{what}: {int(torch.isnan(sums).sum())} NaN sums (a read outside the logical tensor)'
    assert float(sums.abs().max()) > 0, f'{what}: all sums are zero'
    per = 1 if 'bins' in ROUTES[route] else _n_steps(route)  # steps per running sum
    half_ulp = 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11
    np.testing.assert_allclose(sums.numpy().astype(np.float64).sum(-3), per, atol=per * 77 * half_ulp, err_msg=what)


# ---- tap routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('route,mode', ROUTE_MODES)
def test_contiguous_baseline_vs_oracle(route, mode, hw, monkeypatch):
    """L0 on every route: the expected kernel and block size, and the sums against the numpy oracle (the baseline of the strided
    runs must not be wrong in the same way as they are).  Tolerances: tests/test_gpu_parity.py::test_tap_qk_vs_oracle."""
    r = ROUTES[route]
    np_dt, _, accumulate, _ = MODES[mode]
    res = _run(monkeypatch, route, mode, hw, 'L0')
    assert (res['name'], res['block']) == _expected(route, 'L0'), (res['name'], res['block'])
    _check_sane(res, route, mode, f'{route} {mode} hw {hw} L0')
    okey = (r['heads'], r['d'], hw, mode.replace('_strict', '_exact'), 'bins' in r, _n_steps(route))
    if okey not in _oracle_cache:
        acc_np = np.float32 if accumulate == 'float32' else np_dt
        qs, ks = zip(*_data(hw, r['heads'], r['d'], np_dt)[:_n_steps(route)])
        if 'bins' in r:                                       # one step per window
            want = np.stack([_oracle_steps([q], [k], r['heads'], r['d'] ** -0.5, np_dt, acc_np) for q, k in zip(qs, ks)])
        else:
            want = _oracle_steps(qs, ks, r['heads'], r['d'] ** -0.5, np_dt, acc_np)
        _oracle_cache[okey] = want.astype(np.float64)
    want = _oracle_cache[okey]
    got = res['sums'].float().numpy().astype(np.float64)
    assert got.shape == want.shape
    steps = 1 if 'bins' in r else _n_steps(route)
    half_ulp = 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11      # of a probability <= 1
    if mode == 'f32':
        tol = 2e-6 * max(1.0, np.abs(want).max())
    elif accumulate == 'exact':
        tol = 2 * half_ulp * max(1.0, want.max())             # 1 ulp of the largest running sum
    else:
        tol = steps * half_ulp                                # one flipped probability ulp per step
    err = np.abs(got - want).max()
    print(f'{route} {mode} hw {hw}: max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{route} {mode} hw {hw}: max-abs {err} > {tol}'


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('route,mode', ROUTE_MODES)
def test_strided_layout_keeps_every_bit(route, mode, hw, layout, monkeypatch):
    base = _run(monkeypatch, route, mode, hw, 'L0')
    res = _run(monkeypatch, route, mode, hw, layout)
    what = f'{route} {mode} hw {hw} {layout}'
    assert (res['name'], res['block']) == _expected(route, layout), (what, res['name'], res['block'])
    _check_sane(res, route, mode, what)
    assert res['sums'].dtype == base['sums'].dtype and res['sums'].shape == base['sums'].shape
    differ = _bits(res['sums']) != _bits(base['sums'])
    assert not differ.any(), f'{what} ({res["name"]}) vs L0 ({base["name"]}): {int(differ.sum())} of {differ.numel()} sums differ'


@pytest.mark.parametrize('layout', L4)
@pytest.mark.parametrize('route,mode', ROUTE_F16)
def test_layouts_outside_the_predicates_take_the_any_shape_kernel(route, mode, layout, monkeypatch):
    """Row stride c + 4 / an 8-byte aligned pointer, on Q alone or on K alone: no 16-byte piece of such a tensor is aligned, so the
    call must leave every specialised kernel; the any-shape kernel (f32 FMA dot products) then agrees with the route's own kernel
    on L0 within the bound of test_raw_abi_strides_past_32_bit_offsets_fall_back."""
    hw = 576
    base = _run(monkeypatch, route, mode, hw, 'L0')
    res = _run(monkeypatch, route, mode, hw, layout)
    what = f'{route} {mode} hw {hw} {layout}'
    assert (res['name'], res['block']) == _expected(route, layout), (what, res['name'], res['block'])
    _check_sane(res, route, mode, what)
    a, b = res['sums'].float(), base['sums'].float()
    err, tol = float((a - b).abs().max()), 2.0 ** -10 * max(1.0, float(b.max()))
    print(f'{what}: max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, what


# ---- attend ----------------------------------------------------------------------------------------------------------------
ATTEND_CASES = [
    # (torch dtype, head_dim, heads, hw)
    (torch.float16, 64, 2, 576), (torch.float16, 64, 2, 256), (torch.float16, 40, 8, 256), (torch.float16, 160, 2, 256),
    (torch.bfloat16, 64, 2, 576),
]
ATTEND_IDS = ['f16_d64_hw576', 'f16_d64_hw256', 'f16_d40_hw256', 'f16_d160_hw256', 'bf16_d64_hw576']
_attend_cache = {}


def _attend_steps(dtype, d, heads, hw):
    return [_attend_inputs(BATCH, heads, hw, seed=31 * step + d + hw, dtype=dtype, head_dim=d) for step in range(2)]


def _place_call(layout, q, k, v, heads):
    """Q, K, V and a sentinel-filled out of one call in ``layout`` (L1: K and V are the two halves of one buffer)."""
    nan = float('nan')
    pq = _Placed(q, _layout_of(layout, 'q'), 'q', heads, nan)
    pv = _Placed(v, _layout_of(layout, 'v'), 'v', heads, nan)
    pk = _Placed(k, _layout_of(layout, 'k'), 'k', heads, nan, storage=pv.storage if layout == 'L1' else None)
    if layout == 'L1':
        pv.before = pv.storage.clone()                        # the shared buffer now holds K as well
    po = _Placed(torch.full_like(q, OUT_SENTINEL), _layout_of(layout, 'out'), 'out', heads, OUT_SENTINEL)
    return pq, pk, pv, po


def _attend_desc(nat, dtype, heads, hw, d, pq, pk, pv, po):
    return nat.AttendDesc(qk=_qk_desc(nat, dtype, heads, hw, d, pq, pk),
                          v_stride_b=pv.strides[0], v_stride_h=pv.strides[1], v_stride_t=pv.strides[2],
                          o_stride_b=po.strides[0], o_stride_h=po.strides[1], o_stride_p=po.strides[2])


def _out_gaps_intact(po):
    return bool((po.storage[po.gaps] == OUT_SENTINEL).all())


def _attend_run(monkeypatch, case, accumulate, layout):
    """Two ``daam_attend`` calls with the fused tap, then the first call again without it, on ``layout``."""
    key = (case, accumulate, layout)
    if key in _attend_cache:
        return _attend_cache[key]
    from daam_amd import _native as nat
    dtype, d, heads, hw = case
    _configure(monkeypatch, {})
    eng = _raw_engine(dtype, accumulate, heads, hw)
    res = dict(outs=[], supported=[], gaps=[], intact=[])
    calls = [_place_call(layout, q, k, v, heads) for q, k, v in _attend_steps(dtype, d, heads, hw)]
    calls.append(_place_call(layout, *_attend_steps(dtype, d, heads, hw)[0], heads))
    for i, (pq, pk, pv, po) in enumerate(calls):
        desc = _attend_desc(nat, dtype, heads, hw, d, pq, pk, pv, po)
        res['supported'].append(eng.lib.daam_attend_supported(ctypes.byref(desc), pq.ptr, pk.ptr, pv.ptr, po.ptr))
        if i == 2:
            torch.cuda.synchronize()
            res['sums'] = eng.acc[0].clone().cpu()            # after the two tapped calls
        nat.check(eng.lib.daam_attend(eng.ctx, 0, pq.ptr, pk.ptr, pv.ptr, po.ptr, ctypes.byref(desc), 1 if i < 2 else 0, eng.stream))
        torch.cuda.synchronize()
        res['outs'].append(po.logical().cpu())
        res['gaps'].append(_out_gaps_intact(po))
        res['intact'].append(pq.unchanged() and pk.unchanged() and pv.unchanged())
    res['sums_after_untapped'] = eng.acc[0].clone().cpu()
    eng.close()
    _attend_cache[key] = res
    return res


@pytest.mark.parametrize('layout', ('L0',) + LAYOUTS)
@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('case', ATTEND_CASES, ids=ATTEND_IDS)
def test_attend_on_strided_layouts(case, accumulate, layout, monkeypatch):
    dtype, d, heads, hw = case
    base = _attend_run(monkeypatch, case, accumulate, 'L0')
    res = _attend_run(monkeypatch, case, accumulate, layout)
    assert res['supported'] == [1, 1, 1]
    assert all(res['intact']), 'an input storage was written to'
    assert all(res['gaps']), 'a sentinel between the rows of out was overwritten'
    for i, (a, b) in enumerate(zip(res['outs'], base['outs'])):
        assert not torch.isnan(a.float()).any() and not (a == OUT_SENTINEL).all(), i
        assert torch.equal(_bits(a), _bits(b)), f'out of call {i} on {layout} differs from L0: {int((_bits(a) != _bits(b)).sum())} elements'
    assert torch.equal(_bits(res['outs'][2]), _bits(res['outs'][0]))              # the same call with tap = 0
    assert torch.equal(_bits(res['sums_after_untapped']), _bits(res['sums']))     # ... leaves the sums alone
    sums = res['sums']
    assert not torch.isnan(sums.float()).any() and float(sums.float().abs().max()) > 0
    assert torch.equal(_bits(sums), _bits(base['sums'])), f'fused-tap sums on {layout} differ from L0'
    # the stand-alone deferred tap of the same two steps on the same layout
    _configure(monkeypatch, {})
    steps = [(q, k) for q, k, _ in _attend_steps(dtype, d, heads, hw)]
    alone = _tap_raw(steps, heads, d, hw, dtype, accumulate, layout, deferred=True)
    assert alone['intact'] and alone['name'] != 'tap_generic_kernel', alone['name']
    assert torch.equal(_bits(sums), _bits(alone['sums'])), f'fused tap vs stand-alone {alone["name"]} on {layout}'


def test_attend_baseline_matches_reference(monkeypatch):
    """The L0 call of the layout tests against the numpy oracle and the reference's torch ops, as
    tests/test_gpu_attend.py::test_attend_output_matches_reference does (its tolerances)."""
    case = ATTEND_CASES[0]
    dtype, d, heads, hw = case
    res = _attend_run(monkeypatch, case, 'exact', 'L0')
    q, k, v = _attend_steps(dtype, d, heads, hw)[0]
    out = res['outs'][0]
    want_eager, _ = _reference_eager(q, k, v, heads, d ** -0.5)
    scale_v = want_eager.float().abs().max().item()
    # fp16 rounding of the output (2^-11 relative) + an fp16-boundary flip of a logit now and then (summation order)
    assert (out.float() - want_eager.float().cpu()).abs().max().item() <= 2e-3 * scale_v
    want, _ = _restated_f64(q, k, v, heads, d ** -0.5)
    err = (out.float() - want.float()).abs()
    assert err.max().item() <= 2e-3 * scale_v
    ulp = np.spacing(np.abs(want.numpy()).astype(np.float16)).astype(np.float64)
    assert (err.numpy() <= ulp).mean() >= 0.995


@pytest.mark.parametrize('role', ['q', 'k', 'v', 'out'])
@pytest.mark.parametrize('kind', ['L4a', 'L4b'])
def test_attend_declines_layouts_outside_its_predicate(kind, role, monkeypatch):
    """One of the four tensors with a row stride of c + 4 or an 8-byte aligned pointer: daam_attend_supported says no, daam_attend
    returns DAAM_E_UNSUPPORTED and touches neither the sums nor the out storage."""
    from daam_amd import _native as nat
    dtype, d, heads, hw = ATTEND_CASES[1]
    _configure(monkeypatch, {})
    eng = _raw_engine(dtype, 'exact', heads, hw)
    q, k, v = _attend_steps(dtype, d, heads, hw)[0]
    good = _place_call('L0', q, k, v, heads)
    desc = _attend_desc(nat, dtype, heads, hw, d, *good)
    nat.check(eng.lib.daam_attend(eng.ctx, 0, *(p.ptr for p in good), ctypes.byref(desc), 1, eng.stream))
    torch.cuda.synchronize()
    before = eng.acc[0].clone()
    assert float(before.float().abs().max()) > 0
    bad = _place_call(f'{kind}_{role}', q, k, v, heads)
    desc = _attend_desc(nat, dtype, heads, hw, d, *bad)
    assert eng.lib.daam_attend_supported(ctypes.byref(desc), *(p.ptr for p in bad)) == 0
    for tap in (1, 0):
        assert eng.lib.daam_attend(eng.ctx, 0, *(p.ptr for p in bad), ctypes.byref(desc), tap, eng.stream) == nat.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.acc[0]), _bits(before))
    assert bool((bad[3].storage == OUT_SENTINEL).all())
    assert all(p.unchanged() for p in bad[:3])
    eng.close()
