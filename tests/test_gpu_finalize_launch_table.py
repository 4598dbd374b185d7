"""Every finalize launcher picks the instantiation of the context's sums dtype, single and grouped, on every route a switch selects.

The launchers go through one dtype dispatcher (``fin_dispatch``, daam_amd/csrc/daam_finalize.h) and the host through one class table
(``kFinClass``, daam_finalize_api.hip).  A swapped ``DAAM_F32`` / ``DAAM_BF16`` tag compiles, launches and leaves every kernel's machine
code as it was, so byte identity cannot see it.  This file can: per sums dtype one context with layers of side 64 (same size), 32
(x2), 16 (x4), 128 (x0.5) and 24 (any-size kernel), two heads each, a 64 x 64 output and ``n_rows = 3``, finalized once through
``daam_finalize`` and once through ``daam_finalize_groups`` (two groups of one head), on the default route and with
``DAAM_NO_PIPE_FINALIZE`` (fp16), ``DAAM_NO_MFMA_FINALIZE`` and ``DAAM_FORCE_GENERIC`` set; and a context with one 16 x 32 layer and a
32 x 64 output.  Each call must report exactly the expected ``daam_last_kernels`` string and its maps must meet the bound the
existing test of those kernels uses: ``tests/_finalize_domain.py``'s contracts and ``test_gpu_parity.py``'s ``3e-6 * max(1, |want|)``
for the square kernels, ``test_gpu_rect.py``'s per-row bound for the rectangular one.  The planes are multiples of 1 + 2^-9 rounded
to the sums' dtype from a seed of that dtype: the three dtypes hold different numbers, and a kernel reading them as another element
type reads other numbers still.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import _finalize_domain as fd
from oracle import heatmap_oracle as ho
from test_gpu_rect import _assert_rows, _global64

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOKENS, ROWS, HEADS, OUT = 77, 3, 2, 64
SIDES = (64, 32, 16, 128, 24)
CODE = {'f16': 0, 'f32': 1, 'bf16': 2}                          # DAAM_F16 / DAAM_F32 / DAAM_BF16 (include/daam_hip.h)
TORCH_DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
FD_DT = {'f16': 'float16', 'bf16': 'bfloat16', 'f32': 'float32'}
SWITCHES = {'default': None, 'no_pipe': 'DAAM_NO_PIPE_FINALIZE', 'no_mfma': 'DAAM_NO_MFMA_FINALIZE', 'general': 'DAAM_FORCE_GENERIC'}
CASES = [(dt, route) for dt in CODE for route in ('default', 'no_mfma', 'general')] + [('f16', 'no_pipe')]


def expected(dt, route, grouped):
    """``(daam_last_kernels(ctx, 1), an MFMA x2 kernel is among them)``: the classes in launch order -- same size, x4, any size, x0.5, x2
    last (fin_launch_classes)."""
    g = '_grouped' if grouped else ''
    if route == 'general':
        return f'finalize{g}_kernel<{dt}>', False
    rest = [f'finalize_up{g}_kernel<16><{dt}>', f'finalize{g}_kernel<{dt}>', f'finalize_down2{g}_kernel<{dt}>']
    if route == 'no_mfma':
        return '+'.join([f'finalize_same{g}_kernel<{dt}>'] + rest + [f'finalize_up{g}_kernel<32><{dt}>']), False
    if route == 'no_pipe':          # fp16: the round-2 MFMA kernel paired with the same-size class; groups go out as one daam_finalize each
        return '+'.join(rest + ['finalize_up32_same_kernel<f16>']).replace('_grouped', ''), True
    return '+'.join(rest + [f'finalize_up32_pipe{g}_kernel<{dt} + same-size keys>']), True


@lru_cache(maxsize=None)
def _planes(dt, shapes):
    """Per layer ``[HEADS, 77, h, w]`` float32 arrays holding numbers of the sums' dtype; signed, so that the clamp matters."""
    rng = np.random.default_rng([17, CODE[dt]])
    out = []
    for h, w in shapes:
        x = (rng.standard_normal((HEADS, TOKENS, h, w)) * 3).astype(np.float32) * np.float32(1 + 2.0 ** -9)
        x = np.asarray(fd.round_to(x, FD_DT[dt]), np.float32)
        x.setflags(write=False)
        out.append(x)
    return out


@lru_cache(maxsize=None)
def _reference(dt, heads):
    """The float64 oracle over the keys of ``heads`` of every layer, rows [0, ROWS): computed once per dtype and selection, shared."""
    planes = _planes(dt, tuple((s, s) for s in SIDES))
    raw = [((fd.factor_of(s, OUT), layer, h), p[h, :ROWS]) for layer, (s, p) in enumerate(zip(SIDES, planes)) for h in heads]
    want = ho.global_heat_map(raw, OUT * OUT, dtype=np.float64)
    want.setflags(write=False)
    return want


class _Ctx:
    def __init__(self, dt, shapes, out_hw):
        from daam_amd import _native as nat
        self.nat, self.lib, self.out_hw = nat, nat.load(), out_hw
        self.ctx = nat.c_void_p()
        square = out_hw[0] == out_hw[1]
        if square:
            nat.check(self.lib.daam_ctx_create(len(shapes), TOKENS, out_hw[0], CODE[dt], nat.byref(self.ctx)))
        else:
            nat.check(self.lib.daam_ctx_create_rect(len(shapes), TOKENS, out_hw[0], out_hw[1], CODE[dt], nat.byref(self.ctx)))
        self.bufs = []
        for i, ((h, w), p) in enumerate(zip(shapes, _planes(dt, shapes))):
            buf = torch.tensor(p, device=DEV).to(TORCH_DT[dt]).contiguous()
            if square:
                nat.check(self.lib.daam_layer_configure(self.ctx, i, HEADS, h, fd.factor_of(h, out_hw[0]), buf.data_ptr()))
            else:
                nat.check(self.lib.daam_layer_configure_rect(self.ctx, i, HEADS, h, w, max(1, out_hw[0] // h), buf.data_ptr()))
            self.bufs.append(buf)
        self.stream = torch.cuda.current_stream(DEV).cuda_stream

    def kernels(self):
        buf = ctypes.create_string_buffer(512)
        self.nat.check(self.lib.daam_last_kernels(self.ctx, 1, buf, len(buf)))
        return buf.value.decode()

    def single(self):
        out = torch.full((ROWS, *self.out_hw), -1.0, dtype=torch.float32, device=DEV)
        self.nat.check(self.lib.daam_finalize(self.ctx, None, ROWS, out.data_ptr(), self.stream))
        torch.cuda.synchronize()
        return out.cpu().numpy(), self.kernels()

    def groups(self):
        """Two groups: head g of every layer is group g."""
        out = torch.full((HEADS, ROWS, *self.out_hw), -1.0, dtype=torch.float32, device=DEV)
        key_group = (ctypes.c_int32 * (HEADS * len(self.bufs)))(*([0, 1] * len(self.bufs)))
        n_rows = (ctypes.c_int32 * HEADS)(ROWS, ROWS)
        self.nat.check(self.lib.daam_finalize_groups(self.ctx, key_group, HEADS, n_rows, out.data_ptr(), out[0].numel(), self.stream))
        torch.cuda.synchronize()
        return out.cpu().numpy(), self.kernels()

    def close(self):
        self.lib.daam_ctx_destroy(self.ctx)


def _check_square(got, want, mfma, what):
    rel, ab = fd.assert_contract(got, want, mfma, what)
    print(f'\nFINTABLE {what} mfma={int(mfma)} | err_t/rowmax_t <= {rel:.3e} | err_t <= {ab:.3e}')
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-6 * max(1.0, np.abs(want).max()), err_msg=what)


@pytest.mark.parametrize('dt,route', CASES)
def test_square_launch_table(dt, route, monkeypatch):
    for name in SWITCHES.values():                               # read when the native context is created
        if name:
            monkeypatch.setenv(name, '1' if name == SWITCHES[route] else '0')
    c = _Ctx(dt, tuple((s, s) for s in SIDES), (OUT, OUT))
    try:
        got, names = c.single()
        want_names, mfma = expected(dt, route, False)
        assert names == want_names
        _check_square(got, _reference(dt, (0, 1)), mfma, f'{dt} {route} single')
        got, names = c.groups()
        want_names, mfma = expected(dt, route, True)
        assert names == want_names
        for g in range(HEADS):
            _check_square(got[g], _reference(dt, (g,)), mfma, f'{dt} {route} group {g}')
    finally:
        c.close()


@pytest.mark.parametrize('dt', list(CODE))
def test_rect_launch_table(dt):
    shapes, out_hw = ((16, 32),), (32, 64)
    c = _Ctx(dt, shapes, out_hw)
    try:
        p = _planes(dt, shapes)[0]
        got, names = c.single()
        assert names == f'finalize_rect_kernel<{dt}>'
        _assert_rows(got, _global64([p[h, :ROWS] for h in range(HEADS)], *out_hw), f'rect {dt} single')
        got, names = c.groups()
        assert names == f'finalize_rect_grouped_kernel<{dt}>'
        for g in range(HEADS):
            _assert_rows(got[g], _global64([p[g, :ROWS]], *out_hw), f'rect {dt} group {g}')
    finally:
        c.close()
