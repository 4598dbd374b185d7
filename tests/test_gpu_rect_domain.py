"""``finalize_rect_kernel`` / ``finalize_rect_grouped_kernel`` on real key walks, token row by token row against float64
(``tests/_rect_domain.py``: the cases, the levelled rectangular planes, the contract ``err_t <= (2^-19 + max(0, N - 6) * 2^-24) * rowmax_t``
and the host plan; ``tests/test_rect_domain_cpu.py`` holds the reference and the contract themselves).

Every case asserts the kernel name (``daam_last_kernels``), the grid (``daam_last_launch``: token rows x ``plan_chunks`` x groups -- which
makes "this workgroup walked two keys" a checked fact), the contract on every token row of every map, that rows the call does not own
keep their sentinel and that the sums buffers are bit-identical afterwards.  Run with ``-m gpu -s`` on an MI355X: every case prints one
``RECTDOMAIN`` line with its worst ``err_t / rowmax_t`` (DESIGN.md 3.9 records them)."""
import ctypes

import numpy as np
import pytest
import torch

import _finalize_domain as fd
import _rect_domain as rd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -123.0
CODE = {'float16': 0, 'float32': 1, 'bfloat16': 2}
TORCH_DT = {'float16': torch.float16, 'bfloat16': torch.bfloat16, 'float32': torch.float32}


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Ctx:
    """A context made through the rect entry points on the given planes (per layer [heads, 77, h, w], values of ``dtype``), its
    layers' sums in torch buffers of ours."""

    def __init__(self, case, planes, dtype):
        from daam_amd import _native as nat
        self.nat, self.lib = nat, nat.load()
        self.case, self.dtype = case, dtype
        self.out_hw = oh, ow = rd.CASES[case]['out_hw']
        layers = rd.CASES[case]['layers']
        self.ctx = nat.c_void_p()
        nat.check(self.lib.daam_ctx_create_rect(len(layers), rd.TOKENS, oh, ow, CODE[dtype], nat.byref(self.ctx)))
        self.bufs = []
        for i, (((h, w), heads), p) in enumerate(zip(layers, planes)):
            assert p.shape == (heads, rd.TOKENS, h, w)
            buf = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(DEV).to(TORCH_DT[dtype]).contiguous()    # exact: the values are the dtype's
            nat.check(self.lib.daam_layer_configure_rect(self.ctx, i, heads, h, w, max(1, oh // h), buf.data_ptr()))
            self.bufs.append(buf)
        self.before = [b.clone() for b in self.bufs]

    def _stream(self):
        return torch.cuda.current_stream(DEV).cuda_stream

    def run(self, groups, key_mask=None, n_rows=0):
        """One finalize call for ``groups`` (``rd.groups_of``) into sentinel-filled maps [groups, 77, out_h, out_w]; asserts the kernel
        name and the grid; returns the maps on the host."""
        oh, ow = self.out_hw
        out = torch.full((len(groups), rd.TOKENS, oh, ow), SENTINEL, dtype=torch.float32, device=DEV)
        i32 = ctypes.c_int32
        kg = rd.CASES[self.case]['key_group']
        if kg is None:
            m = None if key_mask is None else (ctypes.c_uint8 * len(key_mask))(*key_mask)
            self.nat.check(self.lib.daam_finalize(self.ctx, m, n_rows, out.data_ptr(), self._stream()))
            kernel = 'finalize_rect_kernel'
        else:
            rows = [r for _, r in groups]
            self.nat.check(self.lib.daam_finalize_groups(self.ctx, (i32 * len(kg))(*kg), len(groups), (i32 * len(rows))(*rows), out.data_ptr(),
                                                         rd.TOKENS * oh * ow, self._stream()))
            kernel = 'finalize_rect_grouped_kernel'
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(256)
        self.nat.check(self.lib.daam_last_kernels(self.ctx, 1, buf, len(buf)))
        assert buf.value.decode() == f'{kernel}<{rd.TAG[self.dtype]}>', buf.value
        grid, block, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.nat.check(self.lib.daam_last_launch(self.ctx, 1, ctypes.byref(grid), ctypes.byref(block), ctypes.byref(lds)))
        assert (grid.value, block.value) == (rd.plan_of(groups)[1], 256), (grid.value, block.value, rd.plan_of(groups))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(self.bufs, self.before)), 'a sums buffer was written to'
        return out.cpu().numpy()

    def close(self):
        self.lib.daam_ctx_destroy(self.ctx)


def _judge(got, keys, out_hw, groups, what):
    """The contract on the rows every group owns, the sentinel on the others; the worst ``err_t / rowmax_t``."""
    want = rd.reference(keys, out_hw, groups)
    worst = 0.0
    for g, (idx, rows) in enumerate(groups):
        assert (got[g, rows:] == SENTINEL).all(), f'{what}: group {g} wrote past its {rows} rows'
        worst = max(worst, rd.assert_contract(got[g, :rows], want[g], len(idx), f'{what} group {g}'))
    return worst


def _report(what, groups, worst):
    n_chunks, grid = rd.plan_of(groups)
    print(f'\nRECTDOMAIN device {what} | n_chunks {n_chunks}, grid {grid}, {rd.keys_per_workgroup(groups)} keys per workgroup | '
          f'err_t/rowmax_t <= 2^{rd.log2(worst):.2f}')


@pytest.mark.parametrize('dtype', fd.DTYPES)
@pytest.mark.parametrize('case', list(rd.CASES))
def test_key_walks_vs_float64(case, dtype):
    """Every case of ``rd.CASES``: k = 0 on the signed planes; ``rd.MAGNITUDE_CASES`` at every k of ``fd.K_EXACT`` (+ 40 for bf16 / f32 sums;
    fp16 kept inside its range by ``fd.scale_exp``), non-negative and signed."""
    out_hw = rd.CASES[case]['out_hw']
    groups = rd.groups_of(case)
    runs = [(v, k) for v in fd.VARIANTS for k in rd.exponents(dtype)] if case in rd.MAGNITUDE_CASES else [('signed', 0)]
    if case in ('multi_walk_single', 'one_chunk_groups', 'pieces_mix_16x24', 'pieces_mix_14x6'):
        assert rd.keys_per_workgroup(groups) >= 2                # with the grid asserted in _Ctx.run: a walk of two keys
    worst = 0.0
    for variant, k in runs:
        k, planes = rd.planes_at(case, variant, k, dtype)
        c = _Ctx(case, planes, dtype)
        try:
            got = c.run(groups)
        finally:
            c.close()
        worst = max(worst, _judge(got, rd.key_planes(planes), out_hw, groups, f'{case} {dtype} {variant} k={k}'))
    _report(f'{case} {dtype}', groups, worst)


@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_one_key_per_workgroup_agrees_with_the_walk(dtype):
    """``multi_walk_single``: 77 rows (13 chunks, two keys per workgroup), ``n_rows = 5`` (24 chunks, one key each) and a key mask that
    leaves 14 keys (13 chunks; chunk 0 walks a x2 and then a x4 key).  The short run holds the contract, leaves rows 5 .. 76 alone and
    agrees with the first 5 rows of the long one within twice the contract -- the adds come in another order, so not bit for bit."""
    case, out_hw = 'multi_walk_single', (12, 20)
    _, planes = rd.planes_at(case, 'signed', 0, dtype)
    keys = rd.key_planes(planes)
    c = _Ctx(case, planes, dtype)
    try:
        full, short, masked = rd.groups_of(case), rd.groups_of(case, n_rows=5), rd.groups_of(case, key_mask=rd.KEY_MASK)
        assert (rd.keys_per_workgroup(full), rd.keys_per_workgroup(short), rd.keys_per_workgroup(masked)) == (2, 1, 2)
        got_full = c.run(full)
        got_short = c.run(short, n_rows=5)
        got_masked = c.run(masked, key_mask=rd.KEY_MASK)
    finally:
        c.close()
    _report(f'{case} {dtype} 77 rows', full, _judge(got_full, keys, out_hw, full, f'{case} {dtype} 77 rows'))
    _report(f'{case} {dtype} n_rows=5', short, _judge(got_short, keys, out_hw, short, f'{case} {dtype} n_rows=5'))
    _report(f'{case} {dtype} 14 of 24 keys', masked, _judge(got_masked, keys, out_hw, masked, f'{case} {dtype} 14 of 24 keys'))
    rd.assert_contract(got_short[0, :5], got_full[0, :5].astype(np.float64), 24, f'{case} {dtype}: one key per workgroup against the walk', times=2.0)


@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_one_chunk_groups_twice(dtype):
    """One chunk: one workgroup per (token row, group) and one atomic per element into zeros, so two runs give the same bits."""
    case = 'one_chunk_groups'
    _, planes = rd.planes_at(case, 'signed', 0, dtype)
    groups = rd.groups_of(case)
    assert rd.plan_of(groups) == (1, rd.TOKENS * 12)
    c = _Ctx(case, planes, dtype)
    try:
        first, second = c.run(groups), c.run(groups)
    finally:
        c.close()
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    _judge(first, rd.key_planes(planes), (12, 20), groups, f'{case} {dtype} first of two runs')
